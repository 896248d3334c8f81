"""The device refit (rodent_hip_refit_bvh2_tri1, csrc/build_refit.h; gpubuild.refit_bvh2) on the GPU.

* its nodes, Tri1 records and info words equal tests/refit_model.py's byte for byte after a deformation (Cornell box, seeded soups
  around the block and wave sizes, max_leaf 1 / 2 / 8, LBVH and 3-pass trees, a pre-split tree, a host SBVH tree);
* refitted with the vertices it was built from, an unsplit tree keeps its bytes; a split tree's boxes only grow;
* the refitted atrium tree is traced bit for bit like the oracle (the default kernel's LDS image of the old boxes is stale);
* any stream, reused scratch: the same bytes;
* Renderer.update_geometry renders the moved scene;
* invalid arguments are refused on the host, invalid meshes and malformed hierarchies raise device flags.
"""
import copy
import ctypes as C
import shutil

import numpy as np
import pytest

import refit_model as R
from conftest import GOLDEN
from rodent_amd import formats as F
from rodent_amd import scene as S
from test_gpu_build import soup

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6
SOUPS = (1, 2, 3, 63, 64, 65, 256, 257, 1000, 100003)


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


def refit_equals_model(gb, bvh, moved, ix):
    """Refits `bvh` on the device and its downloaded arrays in the model; asserts equal bytes and info.  Returns the model's result."""
    before = gb.download(bvh)
    model = R.refit(*before, moved, ix)
    out = gb.refit_bvh2(bvh, moved, ix)
    assert out is bvh
    nodes, tris = gb.download(bvh)
    assert bvh.info.tolist() == model[2].tolist() == [bvh.num_nodes, bvh.num_tris, 0, 0]
    assert nodes.tobytes() == model[0].tobytes()
    assert tris.tobytes() == model[1].tobytes()
    assert nodes.tobytes() != before[0].tobytes() or len(ix) == 0
    return model


@pytest.mark.parametrize("passes", (0, 3))
@pytest.mark.parametrize("max_leaf", (1, 2, 8))
def test_bytes_equal_the_model_after_a_deformation(gb, cornell_scene, max_leaf, passes):
    cases = [("cornell", cornell_scene.vertices, cornell_scene.indices)] + [(f"soup{n}", *soup(n, n + max_leaf)) for n in SOUPS]
    for name, v, ix in cases:
        bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes)
        if len(ix) == 1:
            assert gb.download(bvh)[0]["child"].tolist() == [[~0, 0]]        # the single-root form: an empty second slot
        refit_equals_model(gb, bvh, R.deform(v, ix, seed=len(ix) + passes), ix)


@pytest.mark.parametrize("passes", (0, 3))
def test_refit_with_the_builds_own_vertices_is_the_identity(gb, cornell_scene, passes):
    for name, v, ix in (("cornell", cornell_scene.vertices, cornell_scene.indices), ("soup100003", *soup(100003, 100005))):
        bvh = gb.build_bvh2(v, ix, 2, treelet_passes=passes)
        built = gb.download(bvh)
        gb.refit_bvh2(bvh, v, ix)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(built, gb.download(bvh))), name
        assert bvh.info.tolist() == [bvh.num_nodes, bvh.num_tris, 0, 0], name


def test_identity_on_the_atrium(gb, atrium):
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2, treelet_passes=3)
    built = gb.download(bvh)
    gb.refit_bvh2(bvh, atrium.vertices, atrium.indices)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(built, gb.download(bvh)))


def test_split_tree_equals_the_model_and_its_boxes_only_grow(gb, cornell_scene):
    for name, v, ix in (("soup1000", *soup(1000, 1002)), ("cornell", cornell_scene.vertices, cornell_scene.indices)):
        bvh = gb.build_bvh2(v, ix, 2, treelet_passes=3, split_budget=1)
        assert bvh.num_tris > len(ix), name
        built = gb.download(bvh)
        model = R.refit(*built, v, ix)
        gb.refit_bvh2(bvh, v, ix)                                # the build's own vertices: whole-triangle boxes for clipped ones
        nodes, tris = gb.download(bvh)
        assert (nodes.tobytes(), tris.tobytes()) == (model[0].tobytes(), model[1].tobytes()), name
        assert bvh.info.tolist() == model[2].tolist() == [bvh.num_nodes, bvh.num_tris, 0, 0], name
        assert R.contains(nodes, built[0]).all() and tris.tobytes() == built[1].tobytes(), name
        assert nodes.tobytes() != built[0].tobytes(), name
        refit_equals_model(gb, bvh, R.deform(v, ix, seed=9), ix)


def test_host_sbvh_tree_refits_to_the_models_bytes(gb, cornell_scene):
    from rodent_amd import abi
    nodes, tris = F.read_bvh(GOLDEN / "cornell.bvh", F.BVH2_TRI1)
    bvh = abi.DeviceBvh(2, nodes, tris, 0)
    refit_equals_model(gb, bvh, R.deform(cornell_scene.vertices, cornell_scene.indices, seed=2), cornell_scene.indices)


def test_traversal_of_the_refitted_atrium_is_bit_exact(gb, oracle, atrium):
    from rodent_amd import abi, raygen, scenes
    bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2, treelet_passes=1)
    moved = R.deform(atrium.vertices, atrium.indices, seed=1)
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    lo, hi = moved[:, :3].min(0), moved[:, :3].max(0)
    sets = {"primary": raygen.primary_rays(eye, d, up, fov, 256, 256, 0.0, scenes.PRIMARY_TMAX),
            "random": raygen.random_rays(lo, hi, 1 << 16, 7, 0.0, 1.0)}
    single = [v for v in range(len(abi.variants(2))) if "k_bvh2_single" in abi.kernel_name(2, v)][0]
    abi.top_min_rays(0)                           # every default launch through the LDS-image kernel: the image of the old boxes is stale
    try:
        first = {k: abi.traverse(bvh, rays, variant=0) for k, rays in sets.items()}
        gb.refit_bvh2(bvh, moved, atrium.indices)
        nodes, tris = gb.download(bvh)
        for k, rays in sets.items():
            ref, st = oracle.traverse(2, nodes, tris, rays)
            assert st["max_stack"] < 64
            for v in (0, single):
                assert abi.traverse(bvh, rays, variant=v).tobytes() == ref.tobytes(), (k, v)
            assert ref.tobytes() != first[k].tobytes(), k
    finally:
        abi.top_min_rays(-1)


def test_deterministic_across_streams_and_reused_scratch(gb):
    import torch
    v, ix = soup(100003, 100004)
    moved = R.deform(v, ix, seed=3)
    results = []
    big = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").fill_(0xAB)
    for stream, scratch in ((torch.cuda.Stream(), None), (torch.cuda.Stream(), None), (None, big), (None, big)):
        bvh = gb.build_bvh2(v, ix, 2)
        gb.refit_bvh2(bvh, moved, ix, stream=stream, scratch=scratch)
        if scratch is not None:
            assert bvh.scratch is scratch
        results.append(tuple(x.tobytes() for x in gb.download(bvh)))
    assert all(r == results[0] for r in results[1:])


def test_renderer_update_geometry_renders_the_moved_scene(native_build, oracle, cornell_scene, tmp_path):
    from rodent_amd import render as Rn
    lines = (GOLDEN / "cornell_box.obj").read_text().splitlines()
    out = []
    for line in lines:
        if line.startswith("v "):
            x, y, z = (float(c) for c in line.split()[1:4])
            line = "v %.6f %.6f %.6f" % (x + 0.25 * y, y, z + 0.1 * y)          # a shear along y
        out.append(line)
    (tmp_path / "sheared.obj").write_text("\n".join(out) + "\n")
    shutil.copy(GOLDEN / "cornell_box.mtl", tmp_path / "cornell_box.mtl")
    second = S.convert(tmp_path / "sheared.obj", tmp_path / "sheared.rscene")
    assert np.array_equal(second.indices, cornell_scene.indices)
    assert not np.array_equal(second.vertices, cornell_scene.vertices)
    W, H, spp, depth = 64, 64, 4, 6
    cam = S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)
    r = Rn.Renderer(cornell_scene, W, H, spp, depth, gpu_bvh=2)
    try:
        r.render(cam, 0)
        film_first = r.film()
        topology = r.scene_bvh()[0]["child"].copy()
        r.update_geometry(second)
        r.clear()
        r.render(cam, 0)
        film = r.film()
        nodes, tris = r.scene_bvh()
        with pytest.raises(ValueError):
            other = copy.copy(second)
            other.indices = second.indices[::-1].copy()
            r.update_geometry(other)
    finally:
        r.close()
    assert nodes["child"].tobytes() == topology.tobytes()
    refitted = copy.copy(second)
    refitted.nodes, refitted.tris = nodes, tris                  # the second scene under the hierarchy the device traces
    film_o, _ = oracle.render(refitted, cam, 0, spp, depth, W, H)
    assert np.allclose(film, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.01
    assert not np.allclose(film, film_first, rtol=FILM_RTOL, atol=FILM_ATOL)


def seven_node_tree():
    """A complete tree by hand: 7 nodes, 8 leaves of one triangle each, over 8 triangles along x."""
    n = 8
    v = np.zeros((3 * n, 4), np.float32)
    for t in range(n):
        v[3 * t: 3 * t + 3, :3] = np.float32([[2 * t, 0, 0], [2 * t + 1, 0, t], [2 * t, 1, 1]])
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    tris = np.zeros(n, F.TRI1)
    tris["prim_id"] = (np.arange(n) | (1 << 31)).astype(np.uint32).view(np.int32)
    nodes = np.zeros(7, F.NODE2)
    nodes["bounds"][:] = np.float32([np.inf, -np.inf] * 6)
    nodes["child"][:3] = [[2, 3], [4, 5], [6, 7]]
    nodes["child"][3:] = [[~(2 * k), ~(2 * k + 1)] for k in range(4)]
    return v, ix, nodes, tris


def test_refusals_and_flags(gb):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    assert l.rodent_hip_refit_scratch_bytes(0, 1) == -1 and l.rodent_hip_refit_scratch_bytes(1, 0) == -1
    assert l.rodent_hip_refit_scratch_bytes(1, 1) > 0
    v, ix, nodes, tris = seven_node_tree()
    good = abi.DeviceBvh(2, nodes, tris, 0)
    m_nodes, m_tris, m_info = R.refit(nodes, tris, v, ix)
    assert m_info.tolist() == [7, 8, 0, 0]
    # host-side refusals enqueue nothing: the hierarchy and the info words stay as they are
    vd, ixd = torch.from_numpy(v).cuda(), torch.from_numpy(ix).cuda()
    scratch = torch.empty(l.rodent_hip_refit_scratch_bytes(7, 8), dtype=torch.uint8, device="cuda")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda nv=len(v), n=8, nn=7, nt=8, vp=vd.data_ptr(): l.rodent_hip_refit_bvh2_tri1(
        0, vp, nv, ixd.data_ptr(), n, good.nodes.data_ptr(), nn, good.tris.data_ptr(), nt, scratch.data_ptr(), info.data_ptr(), stream)
    assert call(n=0) == -1 and call(n=(1 << 25) + 1) == -1 and call(nv=0) == -3
    assert call(nn=0) == -11 and call(nt=0) == -11 and call(vp=None) == -4
    assert l.rodent_hip_refit_bvh2_tri1(99, vd.data_ptr(), len(v), ixd.data_ptr(), 8, good.nodes.data_ptr(), 7, good.tris.data_ptr(), 8,
                                        scratch.data_ptr(), info.data_ptr(), stream) == -5
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [77] * 4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(good), (nodes, tris)))
    assert call() == 0
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [7, 8, 0, 0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(good), (m_nodes, m_tris)))
    # the sync form, on device pointers too
    host_info = (C.c_int32 * 4)()
    assert l.rodent_hip_refit_bvh2_tri1_sync(0, vd.data_ptr(), len(v), ixd.data_ptr(), 8, good.nodes.data_ptr(), 7, good.tris.data_ptr(),
                                             8, host_info) == 0 and list(host_info) == [7, 8, 0, 0]
    # an index outside the vertex array (spare rows behind `nv`: a missing guard would still read inside the buffer), a NaN
    bad = ix.copy(); bad[5, 1] = len(v)
    spare = torch.from_numpy(np.concatenate([v, np.ones((8, 4), np.float32)])).cuda()
    bad_d = torch.from_numpy(bad).cuda()
    b = abi.DeviceBvh(2, nodes, tris, 0)
    assert l.rodent_hip_refit_bvh2_tri1(0, spare.data_ptr(), len(v), bad_d.data_ptr(), 8, b.nodes.data_ptr(), 7, b.tris.data_ptr(), 8,
                                        scratch.data_ptr(), info.data_ptr(), stream) == 0
    model = R.refit(nodes, tris, v, bad)
    assert info.cpu().tolist() == model[2].tolist() == [7, 8, gb.BAD_INDEX, 0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gb.download(b), model[:2]))       # the vertex read as the origin
    with pytest.raises(gb.BuildError, match="index"):
        gb.refit_bvh2(abi.DeviceBvh(2, nodes, tris, 0), v, bad)
    nan = v.copy(); nan[4, 1] = np.nan
    with pytest.raises(gb.BuildError, match="non-finite"):
        gb.refit_bvh2(abi.DeviceBvh(2, nodes, tris, 0), nan, ix)
    # a child id beyond the node array: flagged, the node and its ancestors stay incomplete, the rest equals the model
    broken = nodes.copy(); broken["child"][2, 1] = 7 + 5
    b = abi.DeviceBvh(2, broken, tris, 0)
    with pytest.raises(gb.BuildError, match="malformed"):
        gb.refit_bvh2(b, v, ix)
    model = R.refit(broken, tris, v, ix)
    assert b.info.tolist() == model[2].tolist() and b.info[2] == gb.BAD_TOPOLOGY and b.info[0] == 5 < 7
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gb.download(b), model[:2]))
    host_info = (C.c_int32 * 4)()
    assert l.rodent_hip_refit_bvh2_tri1_sync(0, vd.data_ptr(), len(v), ixd.data_ptr(), 8, b.nodes.data_ptr(), 7, b.tris.data_ptr(), 8,
                                             host_info) == -7 and host_info[2] == gb.BAD_TOPOLOGY
    # a prim_id beyond the index array: flagged, that record stays as it is
    t2 = tris.copy(); t2["prim_id"][3] = np.int32(-2 ** 31) | np.int32(8)
    b = abi.DeviceBvh(2, nodes, t2, 0)
    with pytest.raises(gb.BuildError, match="malformed"):
        gb.refit_bvh2(b, v, ix)
    model = R.refit(nodes, t2, v, ix)
    assert b.info.tolist() == model[2].tolist() == [7, 7, gb.BAD_TOPOLOGY, 0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gb.download(b), model[:2]))
    # a clean refit afterwards: the flags are per call
    assert gb.refit_bvh2(abi.DeviceBvh(2, nodes, tris, 0), v, ix).info.tolist() == [7, 8, 0, 0]
