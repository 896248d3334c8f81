"""The splitting device builder (triangle pre-splitting: rodent_hip_build_bvh2_tri1_split, include/rodent_build.h) on the GPU.

* its nodes, triangles and all 8 info words equal tests/split_model.py's byte for byte (Cornell box, seeded soups, long slivers, an
  input that leaves allotted splits unmade; budgets 0 ... 4, max_pieces 1, 2, 64, passes 0 and 3, max_leaf 1, 2, 8), on any stream,
  into reused scratch;
* budget 0 is the optimising entry byte for byte, on the atrium too;
* every order-preserving traversal variant on split atrium and plant trees reproduces the oracle bit for bit, and where the answers
  differ from the host SBVH's the ray is ambiguous;
* the renderer's device-built split scene and `rodent --gpu-bvh --treelet-passes 3 --split-budget 1`;
* invalid split options are refused on the host, invalid meshes still raise device flags and leave the allotment finite.
Every tree is downloaded and checked on the host (split_model.check_split_structure) before anything traces or renders it.
"""
import copy
import ctypes as C
import subprocess

import numpy as np
import pytest

import split_model as SM
import trbvh_model as T
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_gpu_build import FILM_ATOL, FILM_RTOL, atrium, cornell_scene, gb, soup  # noqa: F401 (fixtures)
from test_split_model import slivers, sliver_soup_with_unmade_splits

pytestmark = pytest.mark.gpu
SPLITS = [(0.0, 64), (0.25, 64), (1.0, 2), (1.0, 64), (4.0, 1), (4.0, 2), (4.0, 64)]


@pytest.fixture(scope="module")
def plant(native_build, tmp_path_factory):
    from rodent_amd import scenes
    return S.convert(scenes.scene_obj("plant/1"), tmp_path_factory.mktemp("plant") / "plant.rscene")


def checked(gb, bvh, num_tris, max_leaf, max_pieces, passes):
    """Host copies of a built tree, after its structure and depth have been checked."""
    nodes, tris = gb.download(bvh)
    depth = SM.check_split_structure(nodes, tris, num_tris, max_leaf, max_pieces, preorder=passes > 0)
    assert depth == bvh.depth == bvh.info[1] and len(nodes) == bvh.info[0] and len(tris) == bvh.info[4] == bvh.num_tris
    return nodes, tris


def assert_same_bytes(gb, bvh, model, num_tris, max_leaf, max_pieces, passes):
    assert np.array_equal(bvh.info, model[2]), (bvh.info, model[2])
    nodes, tris = checked(gb, bvh, num_tris, max_leaf, max_pieces, passes)
    assert nodes.tobytes() == model[0].tobytes()
    assert tris.tobytes() == model[1].tobytes()


@pytest.mark.parametrize("passes", [0, 3])
@pytest.mark.parametrize("max_leaf", [1, 2, 8])
def test_bytes_equal_the_model(gb, cornell_scene, max_leaf, passes):
    cases = [("cornell", cornell_scene.vertices, cornell_scene.indices)]
    cases += [(f"soup{n}", *soup(n, n + max_leaf)) for n in (1, 2, 3, 65, 256, 257, 1000)]
    cases += [("slivers", *slivers(2000, max_leaf)), ("unmade", *sliver_soup_with_unmade_splits())]
    unmade = 0
    for name, v, ix in cases:
        for budget, pieces in SPLITS:
            bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes, split_budget=budget, max_pieces=pieces)
            model = SM.build(v, ix, max_leaf, passes, budget, pieces)
            try:
                assert_same_bytes(gb, bvh, model, len(ix), max_leaf, pieces, passes)
            except AssertionError as e:
                raise AssertionError(f"{name}, budget {budget}, max_pieces {pieces}: {e}") from e
            unmade += int(bvh.info[6])
    assert unmade > 0, "no input left allotted splits unmade"


def test_deterministic_across_streams_and_reused_scratch(gb, atrium):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    kw = {"treelet_passes": 3, "split_budget": 1.0}
    a = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s1, **kw)
    b = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s2, **kw)
    ref = checked(gb, a, atrium.num_tris, 2, 64, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(b)))
    assert np.array_equal(a.info, b.info) and a.info[5] > 0
    v, ix = slivers(200001, 3, 500.0)
    big = gb.build_bvh2(v, ix, 2, treelet_passes=3, split_budget=4.0)
    checked(gb, big, len(ix), 2, 64, 3)
    c = gb.build_bvh2(atrium.vertices, atrium.indices, 2, scratch=big.scratch, out=big, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(c)))
    model = SM.build(atrium.vertices, atrium.indices, 2, 0, 1.0)
    got = gb.build_bvh2(atrium.vertices, atrium.indices, 2, split_budget=1.0)
    assert_same_bytes(gb, got, model, atrium.num_tris, 2, 64, 0)


def test_budget_zero_is_the_optimising_entry(gb, cornell_scene, atrium):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    for v, ix in ((cornell_scene.vertices, cornell_scene.indices), soup(1000, 7), (atrium.vertices, atrium.indices)):
        n = len(ix)
        vd, ixd = torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(ix)).cuda()
        for max_leaf, passes in ((1, 0), (2, 0), (2, 3), (8, 3)):
            opt = gb.options(max_leaf, passes)
            out = []
            for call, sp in (("opt", None), ("split", gb.split_options(0.0, 64)), ("split", gb.split_options(2.0, 1))):
                assert sp is None or l.rodent_hip_build_split_max_refs(n, C.byref(sp)) == n
                nodes = torch.zeros(max(1, n - 1) * 64, dtype=torch.uint8, device="cuda")
                tris = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
                info = torch.zeros(8, dtype=torch.int32, device="cuda")
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                if call == "opt":
                    scratch = torch.empty(l.rodent_hip_build_opt_scratch_bytes(n, C.byref(opt)), dtype=torch.uint8, device="cuda")
                    rc = l.rodent_hip_build_bvh2_tri1_opt(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, C.byref(opt), nodes.data_ptr(),
                                                          tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), s)
                else:
                    scratch = torch.empty(l.rodent_hip_build_split_scratch_bytes(n, C.byref(opt), C.byref(sp)), dtype=torch.uint8,
                                          device="cuda")
                    rc = l.rodent_hip_build_bvh2_tri1_split(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, C.byref(opt), C.byref(sp),
                                                            nodes.data_ptr(), tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), s)
                assert rc == 0
                words = info.cpu().numpy()
                if call == "split":
                    assert list(words[4:]) == [n, 0, 0, 0]
                out.append((nodes.cpu().numpy().tobytes(), tris.cpu().numpy().tobytes(), words[:4].tobytes()))
            assert out[0] == out[1] == out[2], (n, max_leaf, passes)


@pytest.fixture(scope="module")
def scene_rays(atrium, plant):
    from rodent_amd import raygen, scenes
    out = {}
    for name, sc in (("atrium", atrium), ("plant", plant)):
        eye, d, up, fov = scenes.CAMERAS[name]
        lo, hi = sc.vertices[:, :3].min(0), sc.vertices[:, :3].max(0)
        out[name] = {"primary": raygen.primary_rays(eye, d, up, fov, 512, 512, 0.0, scenes.PRIMARY_TMAX),
                     "random": raygen.random_rays(lo, hi, 1 << 18, 42, 0.0, scenes.RANDOM_TMAX)}
    return out


@pytest.mark.parametrize("passes, budget", [(3, 1.0), (0, 0.25), (3, 4.0)])
@pytest.mark.parametrize("which", ["atrium", "plant"])
def test_traversal_on_split_trees_is_bit_exact_and_agrees_with_the_sbvh(gb, oracle, atrium, plant, scene_rays, which, passes, budget):
    from rodent_amd import abi
    sc = atrium if which == "atrium" else plant
    bvh = gb.build_bvh2(sc.vertices, sc.indices, 2, treelet_passes=passes, split_budget=budget)
    nodes, tris = checked(gb, bvh, sc.num_tris, 2, 64, passes)
    assert bvh.num_tris > sc.num_tris
    for kind, rays in scene_rays[which].items():
        for any_hit in (False, True):
            ref, st = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
            assert st["max_stack"] < 64
            for v in abi.order_preserving_variants(2):
                got = abi.traverse(bvh, rays, any_hit=any_hit, variant=v)
                bad = np.nonzero(got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4))[0]
                assert len(bad) == 0, f"{kind} {abi.variants(2)[v]} any_hit={any_hit}: {len(bad)} rays differ"
        got = abi.traverse(bvh, rays, variant=0)
        sbvh, _ = oracle.traverse(2, sc.nodes, sc.tris, rays)
        diff = np.nonzero((got["tri_id"] != sbvh["tri_id"]) | (got["t"] != sbvh["t"]))[0]
        print(f"{which} {kind}: {len(diff)} of {len(rays)} rays differ between the split GPU tree and the SBVH")
        if len(diff):
            brute, second = oracle.brute_force(sc.tris, rays[diff])
            amb = ambiguous_mask(brute, second)
            assert amb.all(), f"{(~amb).sum()} differing rays are not ambiguous, first {diff[~amb][0]}"


@pytest.mark.parametrize("mapping", ["streaming", "megakernel"])
@pytest.mark.parametrize("which", ["cornell", "atrium"])
def test_renderer_scene_with_a_split_device_hierarchy(gb, oracle, cornell_scene, atrium, which, mapping):
    from rodent_amd import render as R
    from rodent_amd import scenes
    sc = cornell_scene if which == "cornell" else atrium
    if which == "cornell":
        W, H, cam = 160, 120, S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, 160, 120)
    else:
        eye, d, up, fov = scenes.CAMERAS["atrium"]
        W, H, cam = 96, 64, S.camera_settings(eye, d, up, fov, 96, 64)
    pre = gb.build_bvh2(sc.vertices, sc.indices, 2, treelet_passes=3, split_budget=1.0)
    nodes, tris = checked(gb, pre, sc.num_tris, 2, 64, 3)
    r = R.Renderer(sc, W, H, 2, 6, mapping=mapping, gpu_bvh=2, gpu_bvh_passes=3, gpu_bvh_split=1.0)
    got_nodes, got_tris = r.scene_bvh()
    assert got_nodes.tobytes() == nodes.tobytes() and got_tris.tobytes() == tris.tobytes()
    r.render(cam, 0)
    c = r.counters(); film_g = r.film(); r.close()
    built = copy.copy(sc)
    built.nodes, built.tris = got_nodes, got_tris
    film_o, counts = oracle.render(built, cam, 0, 2, 6, W, H)
    assert (c["primary_rays"], c["shadow_rays"]) == (counts[0], counts[1])
    assert np.allclose(film_g, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film_g.mean() > 0.01
    film_s, _ = oracle.render(sc, cam, 0, 2, 6, W, H)                # the host SBVH's scene: the same picture
    assert np.allclose(film_g, film_s, rtol=FILM_RTOL, atol=FILM_ATOL)


def test_rodent_cli_split_budget_matches_the_reference_image(gb, native_build, tmp_path):
    from PIL import Image
    out = tmp_path / "o.png"
    cmd = [native_build.BIN_DIR / "rodent", "--scene", GOLDEN / "cornell_box.obj", "--gpu-bvh", "--treelet-passes", "3",
           "--split-budget", "1", "--bench", "50", "--eye", "0", "1", "2.7", "--dir", "0", "0", "-1", "--up", "0", "1", "0",
           "--width", "1080", "--height", "720", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = np.array(Image.open(out).convert("RGB")).astype(np.float32)
    ref = np.array(Image.open(GOLDEN / "ref-cornell.png").convert("RGB")).astype(np.float32)
    mse = ((img - ref) ** 2).mean() / 255.0 ** 2
    assert mse < 3e-4, mse
    for args, msg in ((["--split-budget", "1"], "--gpu-bvh"), (["--gpu-bvh", "--split-budget", "5"], "--split-budget"),
                      (["--gpu-bvh", "--split-budget", "1", "--max-pieces", "65"], "--max-pieces")):
        bad = subprocess.run([native_build.BIN_DIR / "rodent", "--scene", GOLDEN / "cornell_box.obj", *args, "--bench", "1"],
                             capture_output=True, text=True)
        assert bad.returncode != 0 and msg in bad.stdout + bad.stderr


def test_gpubuild_tool_split_budget(gb, native_build, cornell_scene, tmp_path):
    import sys
    from rodent_amd import formats as F
    S.convert(GOLDEN / "cornell_box.obj", tmp_path / "c.rscene")
    out = tmp_path / "c.bvh"
    subprocess.run([sys.executable, "-m", "rodent_amd.gpubuild", tmp_path / "c.rscene", "-o", out, "--max-leaf", "4",
                    "--treelet-passes", "2", "--split-budget", "1.5", "--max-pieces", "8"], check=True, cwd=native_build.ROOT)
    nodes, tris = F.read_bvh(out, F.BVH2_TRI1)
    m_nodes, m_tris, _ = SM.build(cornell_scene.vertices, cornell_scene.indices, 4, 2, 1.5, 8)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()


def test_invalid_split_options_are_refused_on_the_host(gb):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    opt = gb.options(2, 3)
    for fields in ((-0.5, 64), (4.5, 64), (float("nan"), 64), (float("inf"), 64), (1.0, 0), (1.0, 65), (1.0, -3)):
        sp = abi.SplitOptions(*fields)
        assert l.rodent_hip_build_split_max_refs(100, C.byref(sp)) == -1
        assert l.rodent_hip_build_split_scratch_bytes(100, C.byref(opt), C.byref(sp)) == -1
        assert l.rodent_hip_build_bvh2_tri1_split(0, p, 3, p, 100, C.byref(opt), C.byref(sp), p, p, p, p, None) == -10, fields
        assert l.rodent_hip_build_bvh2_tri1_split_sync(0, p, 3, p, 100, C.byref(opt), C.byref(sp), p, p, None) == -10, fields
    good = abi.SplitOptions(1.0, 64)
    assert l.rodent_hip_build_bvh2_tri1_split(0, p, 3, p, 100, C.byref(opt), None, p, p, p, p, None) == -4
    assert l.rodent_hip_build_bvh2_tri1_split(0, p, 3, p, 100, None, C.byref(good), p, p, p, p, None) == -4
    assert l.rodent_hip_build_bvh2_tri1_split(0, p, 3, p, 0, C.byref(opt), C.byref(good), p, p, p, p, None) == -1
    assert l.rodent_hip_build_split_max_refs(100, C.byref(good)) == 200
    assert l.rodent_hip_build_split_max_refs((1 << 25) - 10, C.byref(abi.SplitOptions(4.0, 64))) == 1 << 25
    torch.cuda.synchronize()
    v, ix = soup(10, 2)
    for kw in ({"split_budget": -1.0}, {"split_budget": 4.5}, {"split_budget": float("nan")}, {"max_pieces": 0},
               {"max_pieces": 65}):
        with pytest.raises(gb.BuildError):
            gb.build_bvh2(v, ix, **{"split_budget": 1.0, **kw})


def test_bad_index_and_nan_raise_device_flags_and_keep_the_allotment_finite(gb):
    import torch
    from rodent_amd import abi
    v, ix = slivers(1000, 4)
    bad = ix.copy(); bad[500, 1] = len(v)
    with pytest.raises(gb.BuildError, match="index"):
        gb.build_bvh2(v, bad, treelet_passes=3, split_budget=1.0)
    nan = v.copy(); nan[1234, 1] = np.nan
    with pytest.raises(gb.BuildError, match="non-finite"):
        gb.build_bvh2(nan, ix, treelet_passes=3, split_budget=1.0)
    n = len(ix)
    sp = gb.split_options(1.0, 64)
    refs = abi.lib().rodent_hip_build_split_max_refs(n, C.byref(sp))
    for verts, index, flag in ((v, bad, gb.BAD_INDEX), (nan, ix, gb.NON_FINITE)):
        info = (C.c_int32 * 8)()
        vd, bd = torch.from_numpy(verts).cuda(), torch.from_numpy(index).cuda()
        nodes = torch.empty((refs - 1) * 64, dtype=torch.uint8, device="cuda")
        tris = torch.empty(refs * 48, dtype=torch.uint8, device="cuda")
        rc = abi.lib().rodent_hip_build_bvh2_tri1_split_sync(0, vd.data_ptr(), len(verts), bd.data_ptr(), n, C.byref(gb.options(2, 3)),
                                                             C.byref(sp), nodes.data_ptr(), tris.data_ptr(), info)
        assert rc == -7 and info[2] == flag
        # the flagged triangle has p = 0: the rest is split exactly as the model splits it, within the budget
        model = SM.build(verts, index, 2, 3, 1.0, 64)[2]
        assert list(info)[4:] == list(model[4:]) and n < info[4] <= refs and info[5] > 0
    assert gb.build_bvh2(v, ix, treelet_passes=3, split_budget=1.0).info[2] == 0
