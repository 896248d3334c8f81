"""The optimising device builder (treelet restructuring + SAH leaf collapse: rodent_hip_build_bvh2_tri1_opt, include/rodent_build.h)
on the GPU.

* its nodes, triangles and info words equal tests/trbvh_model.py's byte for byte (Cornell box, seeded soups with degenerate
  triangles, shared centroids and a flat axis, the atrium; passes 1 ... 3, max_leaf 1, 2, 4, 8), on any stream, into reused scratch;
* treelet_passes = 0 is the LBVH entry, byte for byte;
* every order-preserving traversal variant on the optimised atrium tree reproduces the oracle bit for bit, and where its answers
  differ from the host SBVH's the ray is ambiguous;
* the renderer's device-built scene with passes and `rodent --gpu-bvh --treelet-passes 2`;
* invalid options are refused on the host, invalid meshes still raise device flags.
Every tree is downloaded and checked on the host (trbvh_model.check_structure: structure, leaf sizes, depth <= 56) before anything
traces or renders it.
"""
import copy
import ctypes as C
import subprocess

import numpy as np
import pytest

import lbvh_model as L
import trbvh_model as T
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_gpu_build import FILM_ATOL, FILM_RTOL, atrium, cornell_scene, gb, soup  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
MAX_LEAVES = (1, 2, 4, 8)
PASSES = (1, 2, 3)


def checked(gb, bvh, num_tris, max_leaf):
    """Host copies of a built tree, after its structure and depth have been checked."""
    nodes, tris = gb.download(bvh)
    depth = T.check_structure(nodes, tris, num_tris, max_leaf)
    assert depth == bvh.depth == bvh.info[1] and len(nodes) == bvh.info[0]
    return nodes, tris


def assert_same_bytes(gb, bvh, model, num_tris, max_leaf):
    assert np.array_equal(bvh.info, model[2]), (bvh.info, model[2])
    nodes, tris = checked(gb, bvh, num_tris, max_leaf)
    assert nodes.tobytes() == model[0].tobytes()
    assert tris.tobytes() == model[1].tobytes()


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_bytes_equal_the_model_cornell_and_soups(gb, cornell_scene, max_leaf, passes):
    cases = [("cornell", cornell_scene.vertices, cornell_scene.indices)]
    cases += [(f"soup{n}", *soup(n, n + max_leaf)) for n in (1, 2, 3, 8, 63, 64, 65, 256, 257, 1000, 20001)]
    for name, v, ix in cases:
        bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes)
        try:
            assert_same_bytes(gb, bvh, T.build(v, ix, max_leaf, passes), len(ix), max_leaf)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("passes", PASSES)
def test_bytes_equal_the_model_atrium(gb, atrium, passes):
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2, treelet_passes=passes)
    assert_same_bytes(gb, bvh, T.build(atrium.vertices, atrium.indices, 2, passes), atrium.num_tris, 2)


@pytest.mark.parametrize("max_leaf", [1, 2])
def test_bytes_equal_the_model_where_the_depth_rule_rejects(gb, max_leaf):
    from test_gpu_build_opt_model import deep_input
    v, ix = deep_input(20000, 13)
    for passes in PASSES:
        model = T.build(v, ix, max_leaf, passes)
        bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes)
        assert_same_bytes(gb, bvh, model, len(ix), max_leaf)
        assert bvh.depth <= T.MAX_DEPTH
    if max_leaf == 1:
        assert bvh.info[3] > 0, "the input no longer reaches the depth rule"


def test_passes_zero_is_the_lbvh_entry(gb, cornell_scene, atrium):
    from rodent_amd import abi
    import torch
    l = abi.lib()
    for v, ix in ((cornell_scene.vertices, cornell_scene.indices), soup(1000, 7), (atrium.vertices, atrium.indices)):
        for max_leaf in MAX_LEAVES:
            n = len(ix)
            opt = gb.options(max_leaf, 0)
            assert l.rodent_hip_build_opt_scratch_bytes(n, C.byref(opt)) == l.rodent_hip_build_scratch_bytes(n)
            vd, ixd = torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(ix)).cuda()
            out = []
            for call in ("lbvh", "opt"):
                nodes = torch.zeros(max(1, n - 1) * 64, dtype=torch.uint8, device="cuda")
                tris = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
                info = torch.zeros(4, dtype=torch.int32, device="cuda")
                scratch = torch.empty(l.rodent_hip_build_scratch_bytes(n), dtype=torch.uint8, device="cuda")
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                if call == "lbvh":
                    rc = l.rodent_hip_build_bvh2_tri1(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, max_leaf, nodes.data_ptr(),
                                                      tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), s)
                else:
                    rc = l.rodent_hip_build_bvh2_tri1_opt(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, C.byref(opt), nodes.data_ptr(),
                                                          tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), s)
                assert rc == 0
                out.append(tuple(x.cpu().numpy().tobytes() for x in (nodes, tris, info)))
            assert out[0] == out[1]


def test_deterministic_across_streams_and_reused_scratch(gb, atrium):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s1, treelet_passes=3)
    b = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s2, treelet_passes=3)
    ref = checked(gb, a, atrium.num_tris, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(b)))
    assert np.array_equal(a.info, b.info)
    v, ix = soup(300001, 3)
    big = gb.build_bvh2(v, ix, 2, treelet_passes=3)
    checked(gb, big, len(ix), 2)
    c = gb.build_bvh2(atrium.vertices, atrium.indices, 2, scratch=big.scratch, out=big, treelet_passes=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(c)))


@pytest.fixture(scope="module")
def atrium_rays(native_build):
    from rodent_amd import formats as F
    from rodent_amd import raygen, scenes
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    n4, _ = F.read_bvh(scenes.scene_bvh("atrium"), F.BVH4_TRI4)
    lo, hi = raygen.scene_bounds(n4)
    return {"primary": raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX),
            "random": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX)}


@pytest.fixture(scope="module")
def atrium_opt(gb, atrium):
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2, treelet_passes=2)
    return bvh, checked(gb, bvh, atrium.num_tris, 2)


@pytest.mark.parametrize("kind", ["primary", "random"])
def test_traversal_on_the_optimised_atrium_is_bit_exact(oracle, atrium_opt, atrium_rays, kind):
    from rodent_amd import abi
    bvh, (nodes, tris) = atrium_opt
    rays = atrium_rays[kind]
    for any_hit in (False, True):
        ref, st = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
        assert st["max_stack"] < 64
        for v in abi.order_preserving_variants(2):
            got = abi.traverse(bvh, rays, any_hit=any_hit, variant=v)
            bad = np.nonzero(got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4))[0]
            assert len(bad) == 0, f"{abi.variants(2)[v]} any_hit={any_hit}: {len(bad)} rays differ"


@pytest.mark.parametrize("kind", ["primary", "random"])
def test_same_answers_as_the_sbvh_up_to_ambiguous_rays(oracle, atrium, atrium_opt, atrium_rays, kind):
    from rodent_amd import abi
    bvh, (_, tris) = atrium_opt
    rays = atrium_rays[kind]
    got = abi.traverse(bvh, rays, variant=0)
    sbvh, _ = oracle.traverse(2, atrium.nodes, atrium.tris, rays)
    diff = np.nonzero((got["tri_id"] != sbvh["tri_id"]) | (got["t"] != sbvh["t"]))[0]
    print(f"{kind}: {len(diff)} of {len(rays)} rays differ between the optimised GPU tree and the SBVH")
    if len(diff):
        brute, second = oracle.brute_force(tris, rays[diff])
        amb = ambiguous_mask(brute, second)
        assert amb.all(), f"{(~amb).sum()} differing rays are not ambiguous, first {diff[~amb][0]}"


@pytest.mark.parametrize("mapping", ["streaming", "megakernel"])
@pytest.mark.parametrize("which", ["cornell", "atrium"])
def test_renderer_scene_with_an_optimised_device_hierarchy(gb, oracle, cornell_scene, atrium, which, mapping):
    from rodent_amd import render as R
    from rodent_amd import scenes
    sc = cornell_scene if which == "cornell" else atrium
    if which == "cornell":
        W, H, cam = 160, 120, S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, 160, 120)
    else:
        eye, d, up, fov = scenes.CAMERAS["atrium"]
        W, H, cam = 96, 64, S.camera_settings(eye, d, up, fov, 96, 64)
    # the tree the renderer will build, checked on the host first
    m_nodes, m_tris, _ = T.build(sc.vertices, sc.indices, 2, 2)
    T.check_structure(m_nodes, m_tris, sc.num_tris, 2)
    pre = gb.build_bvh2(sc.vertices, sc.indices, 2, treelet_passes=2)
    nodes, tris = checked(gb, pre, sc.num_tris, 2)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()
    r = R.Renderer(sc, W, H, 2, 6, mapping=mapping, gpu_bvh=2, gpu_bvh_passes=2)
    got_nodes, got_tris = r.scene_bvh()
    assert got_nodes.tobytes() == m_nodes.tobytes() and got_tris.tobytes() == m_tris.tobytes()
    r.render(cam, 0)
    c = r.counters(); film_g = r.film(); r.close()
    built = copy.copy(sc)
    built.nodes, built.tris = got_nodes, got_tris
    film_o, counts = oracle.render(built, cam, 0, 2, 6, W, H)
    assert (c["primary_rays"], c["shadow_rays"]) == (counts[0], counts[1])
    assert np.allclose(film_g, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film_g.mean() > 0.01


def test_rodent_cli_treelet_passes_matches_the_reference_image(gb, native_build, cornell_scene, tmp_path):
    from PIL import Image
    bvh = gb.build_bvh2(cornell_scene.vertices, cornell_scene.indices, 2, treelet_passes=2)
    checked(gb, bvh, cornell_scene.num_tris, 2)
    out = tmp_path / "o.png"
    cmd = [native_build.BIN_DIR / "rodent", "--scene", GOLDEN / "cornell_box.obj", "--gpu-bvh", "--treelet-passes", "2", "--bench",
           "50", "--eye", "0", "1", "2.7", "--dir", "0", "0", "-1", "--up", "0", "1", "0", "--width", "1080", "--height", "720", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = np.array(Image.open(out).convert("RGB")).astype(np.float32)
    ref = np.array(Image.open(GOLDEN / "ref-cornell.png").convert("RGB")).astype(np.float32)
    mse = ((img - ref) ** 2).mean() / 255.0 ** 2
    assert mse < 3e-4, mse
    bad = subprocess.run([native_build.BIN_DIR / "rodent", "--scene", GOLDEN / "cornell_box.obj", "--treelet-passes", "2", "--bench",
                          "1"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--gpu-bvh" in bad.stdout + bad.stderr


def test_gpubuild_tool_treelet_passes(gb, native_build, cornell_scene, tmp_path):
    import sys
    from rodent_amd import formats as F
    S.convert(GOLDEN / "cornell_box.obj", tmp_path / "c.rscene")
    out = tmp_path / "c.bvh"
    subprocess.run([sys.executable, "-m", "rodent_amd.gpubuild", tmp_path / "c.rscene", "-o", out, "--max-leaf", "4",
                    "--treelet-passes", "2"], check=True, cwd=native_build.ROOT)
    nodes, tris = F.read_bvh(out, F.BVH2_TRI1)
    m_nodes, m_tris, _ = T.build(cornell_scene.vertices, cornell_scene.indices, 4, 2)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()


def test_invalid_options_are_refused_on_the_host(gb):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    bad = [((0, 1, 1.2, 1.0), -2), ((9, 1, 1.2, 1.0), -2), ((2, -1, 1.2, 1.0), -8), ((2, 4, 1.2, 1.0), -8),
           ((2, 1, 0.0, 1.0), -9), ((2, 1, 1.2, -1.0), -9), ((2, 1, float("nan"), 1.0), -9), ((2, 1, 1.2, float("inf")), -9)]
    for fields, code in bad:
        opt = abi.BuildOptions(*fields)
        assert l.rodent_hip_build_opt_scratch_bytes(100, C.byref(opt)) == -1
        assert l.rodent_hip_build_bvh2_tri1_opt(0, p, 3, p, 100, C.byref(opt), p, p, p, p, None) == code, fields
        assert l.rodent_hip_build_bvh2_tri1_opt_sync(0, p, 3, p, 100, C.byref(opt), p, p, None) == code, fields
    assert l.rodent_hip_build_bvh2_tri1_opt(0, p, 3, p, 100, None, p, p, p, p, None) == -4
    good = abi.BuildOptions(2, 2, 1.2, 1.0)
    assert l.rodent_hip_build_opt_scratch_bytes(0, C.byref(good)) == -1
    assert l.rodent_hip_build_opt_scratch_bytes(100, C.byref(good)) > l.rodent_hip_build_scratch_bytes(100)
    assert l.rodent_hip_build_bvh2_tri1_opt(0, p, 3, p, 0, C.byref(good), p, p, p, p, None) == -1
    torch.cuda.synchronize()
    v, ix = soup(10, 2)
    for kw in ({"treelet_passes": 4}, {"treelet_passes": -1}, {"node_cost": 0.0}, {"tri_cost": float("nan")}, {"max_leaf": 9}):
        with pytest.raises(gb.BuildError):
            gb.build_bvh2(v, ix, **{"treelet_passes": 1, **kw})


def test_bad_index_and_nan_raise_device_flags(gb):
    import torch
    from rodent_amd import abi
    v, ix = soup(1000, 4)
    bad = ix.copy(); bad[500, 1] = len(v)
    with pytest.raises(gb.BuildError, match="index"):
        gb.build_bvh2(v, bad, treelet_passes=2)
    nan = v.copy(); nan[1234, 1] = np.nan
    with pytest.raises(gb.BuildError, match="non-finite"):
        gb.build_bvh2(nan, ix, treelet_passes=2)
    info = (C.c_int32 * 4)()
    vd, bd = torch.from_numpy(v).cuda(), torch.from_numpy(bad).cuda()
    n = len(ix)
    nodes = torch.empty((n - 1) * 64, dtype=torch.uint8, device="cuda")
    tris = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    rc = abi.lib().rodent_hip_build_bvh2_tri1_opt_sync(0, vd.data_ptr(), len(v), bd.data_ptr(), n, C.byref(gb.options(2, 2)),
                                                       nodes.data_ptr(), tris.data_ptr(), info)
    assert rc == -7 and info[2] == gb.BAD_INDEX
    assert gb.build_bvh2(v, ix, treelet_passes=2).info[2] == 0
