"""The device BVH builder (csrc/bvh_build.hip, include/rodent_build.h) on the GPU.

* its nodes, triangles and info words equal tests/lbvh_model.py's byte for byte (Cornell box, seeded soups with degenerate triangles,
  shared centroids and a flat axis, the atrium; max_leaf 1, 2, 4, 8), on any stream, into reused scratch;
* every order-preserving traversal variant on the built atrium tree reproduces the oracle bit for bit, and where its answers differ
  from the host SBVH's the ray is ambiguous (two triangles within 1e-4 in t);
* rebuilt in place, the new tree is traced correctly (the default kernel's LDS image of the old one is stale);
* the renderer's device-built scene and `rodent --gpu-bvh`;
* invalid arguments are refused on the host, invalid meshes raise device flags.
"""
import subprocess

import numpy as np
import pytest

import lbvh_model as L
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import formats as F
from rodent_amd import scene as S

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6
MAX_LEAVES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def gb(native_build):
    import torch
    from rodent_amd import gpubuild
    assert torch.cuda.is_available(), "these tests need a GPU"
    return gpubuild


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


@pytest.fixture(scope="module")
def atrium(native_build, tmp_path_factory):
    from rodent_amd import scenes
    return S.convert(scenes.scene_obj("atrium"), tmp_path_factory.mktemp("atrium") / "atrium.rscene")


def soup(n, seed):
    """n triangles over 3n vertices with every awkward case mixed in: degenerate triangles (a point, a line), pairs with one shared
    centroid, and a flat z axis when `seed` is odd."""
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), np.float32)
    v[:, :3] = rng.uniform(-50, 50, (3 * n, 3)).astype(np.float32)
    if seed % 2:
        v[:, 2] = 7.0
    pts = np.arange(0, n, 7)                                     # degenerate: all three corners in one point
    v[3 * pts + 1], v[3 * pts + 2] = v[3 * pts], v[3 * pts]
    lines = np.arange(3, n, 11)                                  # degenerate: a line
    v[3 * lines + 2] = v[3 * lines + 1]
    dup = np.arange(1, n, 5)                                     # the previous triangle's corners in another order: same centroid
    v[3 * dup], v[3 * dup + 1], v[3 * dup + 2] = v[3 * dup - 3], v[3 * dup - 1], v[3 * dup - 2]
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    ix[:, 3] = rng.integers(0, 5, n)
    return v, ix


def assert_same_bytes(bvh, gb, model):
    nodes, tris = gb.download(bvh)
    m_nodes, m_tris, m_info = model
    assert np.array_equal(bvh.info, m_info), (bvh.info, m_info)
    assert nodes.tobytes() == m_nodes.tobytes()
    assert tris.tobytes() == m_tris.tobytes()


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_bytes_equal_the_model_cornell_and_soups(gb, cornell_scene, max_leaf):
    cases = [("cornell", cornell_scene.vertices, cornell_scene.indices)]
    cases += [(f"soup{n}", *soup(n, n + max_leaf)) for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 100003)]
    for name, v, ix in cases:
        model = L.build(v, ix, max_leaf)
        bvh = gb.build_bvh2(v, ix, max_leaf)
        assert_same_bytes(bvh, gb, model)
        assert bvh.depth <= L.depth_bound(len(ix)), name


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_bytes_equal_the_model_atrium(gb, atrium, max_leaf):
    model = L.build(atrium.vertices, atrium.indices, max_leaf)
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, max_leaf)
    assert_same_bytes(bvh, gb, model)
    assert bvh.depth <= L.depth_bound(atrium.num_tris)


def test_inputs_as_tensors_and_three_columns(gb, cornell_scene):
    import torch
    v = torch.from_numpy(cornell_scene.vertices[:, :3].copy()).cuda()
    ix = torch.from_numpy(cornell_scene.indices[:, :3].copy()).cuda()
    ix4 = cornell_scene.indices.copy()
    ix4[:, 3] = 0
    assert_same_bytes(gb.build_bvh2(v, ix), gb, L.build(cornell_scene.vertices, ix4, 2))


def test_deterministic_across_streams_and_reused_scratch(gb, atrium):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s1)
    b = gb.build_bvh2(atrium.vertices, atrium.indices, 2, stream=s2)
    ref = gb.download(a)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(b)))
    # scratch and output buffers of another (larger) build, then this one again into them
    v, ix = soup(300001, 3)
    big = gb.build_bvh2(v, ix, 2)
    c = gb.build_bvh2(atrium.vertices, atrium.indices, 2, scratch=big.scratch, out=big)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(c)))


@pytest.fixture(scope="module")
def atrium_rays(native_build):
    from rodent_amd import raygen, scenes
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    n4, _ = F.read_bvh(scenes.scene_bvh("atrium"), F.BVH4_TRI4)
    lo, hi = raygen.scene_bounds(n4)
    return {"primary": raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX),
            "random": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX)}


@pytest.mark.parametrize("kind", ["primary", "random"])
def test_traversal_on_the_built_atrium_is_bit_exact(gb, oracle, atrium, atrium_rays, kind):
    from rodent_amd import abi
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2)
    nodes, tris = gb.download(bvh)
    rays = atrium_rays[kind]
    for any_hit in (False, True):
        ref, st = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
        assert st["max_stack"] < 64
        for v in abi.order_preserving_variants(2):
            got = abi.traverse(bvh, rays, any_hit=any_hit, variant=v)
            bad = np.nonzero(got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4))[0]
            assert len(bad) == 0, f"{abi.variants(2)[v]} any_hit={any_hit}: {len(bad)} rays differ"


def test_cornell_golden_rays_on_the_built_tree(gb, oracle, cornell, cornell_scene):
    from rodent_amd import abi
    bvh = gb.build_bvh2(cornell_scene.vertices, cornell_scene.indices, 2)
    nodes, tris = gb.download(bvh)
    for name, rays in cornell.ray_sets.items():
        for any_hit in (False, True):
            ref, _ = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
            for v in abi.order_preserving_variants(2):
                assert abi.traverse(bvh, rays, any_hit=any_hit, variant=v).tobytes() == ref.tobytes(), (name, any_hit, v)


@pytest.mark.parametrize("kind", ["primary", "random"])
def test_same_answers_as_the_sbvh_up_to_ambiguous_rays(gb, oracle, atrium, atrium_rays, kind):
    from rodent_amd import abi
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2)
    rays = atrium_rays[kind]
    got = abi.traverse(bvh, rays, variant=0)
    sbvh, _ = oracle.traverse(2, atrium.nodes, atrium.tris, rays)
    diff = np.nonzero((got["tri_id"] != sbvh["tri_id"]) | (got["t"] != sbvh["t"]))[0]
    print(f"{kind}: {len(diff)} of {len(rays)} rays differ between the GPU tree and the SBVH")
    if len(diff):
        _, tris = gb.download(bvh)                               # one record per triangle (the SBVH's spatial splits repeat some)
        brute, second = oracle.brute_force(tris, rays[diff])
        amb = ambiguous_mask(brute, second)
        assert amb.all(), f"{(~amb).sum()} differing rays are not ambiguous, first {diff[~amb][0]}"


def test_rebuild_in_place_traces_the_new_geometry(gb, oracle, atrium, cornell_scene):
    from rodent_amd import abi, raygen
    a = gb.build_bvh2(atrium.vertices, atrium.indices, 2)
    lo, hi = atrium.vertices[:, :3].min(0), atrium.vertices[:, :3].max(0)
    rays = raygen.random_rays(lo, hi, 1 << 16, 7, 0.0, 1.0)
    abi.top_min_rays(0)                           # every launch through the LDS-image kernel: the image of the first tree is then stale
    try:
        first = abi.traverse(a, rays, variant=0)
        ref, _ = oracle.traverse(2, *gb.download(a), rays)
        assert first.tobytes() == ref.tobytes()
        # other geometry (the atrium scaled and shifted, half of its triangles) into the same buffers
        v = atrium.vertices.copy()
        v[:, :3] = v[:, :3] * np.float32(0.75) + np.float32(40.0)
        ix = atrium.indices[::2].copy()
        b = gb.build_bvh2(v, ix, 2, scratch=a.scratch, out=a)
        assert b.nodes.data_ptr() == a.nodes.data_ptr() and b.tris.data_ptr() == a.tris.data_ptr()
        again = abi.traverse(b, rays, variant=0)
        nodes, tris = gb.download(b)
        assert (nodes.tobytes(), tris.tobytes()) == tuple(x.tobytes() for x in L.build(v, ix, 2)[:2])
        ref2, _ = oracle.traverse(2, nodes, tris, rays)
        assert again.tobytes() == ref2.tobytes()
        assert again.tobytes() != first.tobytes()
    finally:
        abi.top_min_rays(-1)


@pytest.mark.parametrize("mapping", ["streaming", "megakernel"])
@pytest.mark.parametrize("which", ["cornell", "atrium"])
def test_renderer_scene_with_a_device_built_hierarchy(native_build, oracle, cornell_scene, atrium, which, mapping):
    import copy
    from rodent_amd import render as R
    from rodent_amd import scenes
    sc = cornell_scene if which == "cornell" else atrium
    if which == "cornell":
        W, H, cam = 160, 120, S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, 160, 120)
    else:
        eye, d, up, fov = scenes.CAMERAS["atrium"]
        W, H, cam = 96, 64, S.camera_settings(eye, d, up, fov, 96, 64)
    r = R.Renderer(sc, W, H, 2, 6, mapping=mapping, gpu_bvh=2)
    nodes, tris = r.scene_bvh()
    m_nodes, m_tris, _ = L.build(sc.vertices, sc.indices, 2)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()
    r.render(cam, 0)
    c = r.counters(); film_g = r.film(); r.close()
    built = copy.copy(sc)
    built.nodes, built.tris = nodes, tris
    film_o, counts = oracle.render(built, cam, 0, 2, 6, W, H)
    assert (c["primary_rays"], c["shadow_rays"]) == (counts[0], counts[1])
    assert np.allclose(film_g, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film_g.mean() > 0.01


def test_rodent_cli_gpu_bvh_matches_the_reference_image(native_build, tmp_path):
    from PIL import Image
    out = tmp_path / "o.png"
    r = subprocess.run([native_build.BIN_DIR / "rodent", "--scene", GOLDEN / "cornell_box.obj", "--gpu-bvh", "--bench", "50",
                        "--eye", "0", "1", "2.7", "--dir", "0", "0", "-1", "--up", "0", "1", "0", "--width", "1080", "--height", "720",
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = np.array(Image.open(out).convert("RGB")).astype(np.float32)
    ref = np.array(Image.open(GOLDEN / "ref-cornell.png").convert("RGB")).astype(np.float32)
    mse = ((img - ref) ** 2).mean() / 255.0 ** 2
    assert mse < 3e-4, mse


def test_invalid_arguments_are_refused_on_the_host(gb, native_build):
    import ctypes as C
    import torch
    from rodent_amd import abi
    l = abi.lib()
    assert l.rodent_hip_build_scratch_bytes(0) == -1 and l.rodent_hip_build_scratch_bytes((1 << 25) + 1) == -1
    assert l.rodent_hip_build_scratch_bytes(1 << 25) > 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    call = lambda n, ml: l.rodent_hip_build_bvh2_tri1(0, p, 3, p, n, ml, p, p, p, p, None)
    assert call(0, 2) == -1 and call((1 << 25) + 1, 2) == -1
    assert call(1, 0) == -2 and call(1, 9) == -2
    assert l.rodent_hip_build_bvh2_tri1(0, p, 3, None, 1, 2, p, p, p, p, None) == -4
    torch.cuda.synchronize()
    v, ix = soup(10, 2)
    for kw in ({"max_leaf": 0}, {"max_leaf": 9}):
        with pytest.raises(gb.BuildError):
            gb.build_bvh2(v, ix, **kw)
    with pytest.raises(gb.BuildError):
        gb.build_bvh2(v, ix[:0])


def test_bad_index_and_nan_raise_device_flags(gb):
    import torch
    from rodent_amd import abi
    v, ix = soup(1000, 4)
    nv = len(v)
    # the vertex buffer has spare rows behind the `nv` the builder is told about: a missing guard would still read inside it
    spare = torch.from_numpy(np.concatenate([v, np.ones((64, 4), np.float32)])).cuda()
    bad = ix.copy(); bad[500, 1] = nv
    ix_d = torch.from_numpy(bad).cuda()
    n = len(ix)
    scratch = torch.empty(abi.lib().rodent_hip_build_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    nodes = torch.empty((n - 1) * 64, dtype=torch.uint8, device="cuda")
    tris = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    import ctypes as C
    rc = abi.lib().rodent_hip_build_bvh2_tri1(0, spare.data_ptr(), nv, ix_d.data_ptr(), n, 2, nodes.data_ptr(), tris.data_ptr(),
                                              scratch.data_ptr(), info.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert info.cpu().numpy()[2] == gb.BAD_INDEX
    with pytest.raises(gb.BuildError, match="index"):
        gb.build_bvh2(v, bad)
    nan = v.copy(); nan[1234, 1] = np.nan
    with pytest.raises(gb.BuildError, match="non-finite"):
        gb.build_bvh2(nan, ix)
    # a clean build afterwards: the flags are per call
    assert gb.build_bvh2(v, ix).info[2] == 0


def test_gpubuild_tool_writes_a_bvh_file(native_build, cornell_scene, tmp_path):
    import sys
    S.convert(GOLDEN / "cornell_box.obj", tmp_path / "c.rscene")
    out = tmp_path / "c.bvh"
    subprocess.run([sys.executable, "-m", "rodent_amd.gpubuild", tmp_path / "c.rscene", "-o", out, "--max-leaf", "4"], check=True,
                   cwd=native_build.ROOT)
    nodes, tris = F.read_bvh(out, F.BVH2_TRI1)
    m_nodes, m_tris, _ = L.build(cornell_scene.vertices, cornell_scene.indices, 4)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()
