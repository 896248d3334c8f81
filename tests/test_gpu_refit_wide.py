"""The device refit of the wide layouts (rodent_hip_refit_bvh4_tri4 / _bvh8_tri4, csrc/build_refit.h; gpubuild.refit_wide) on the GPU.

* nodes, Tri4 packets and info words equal tests/refit_wide_model.py's byte for byte after a deformation: the Cornell blocks, the
  hand-made trees of test_refit_wide_model.py, host-built trees of seeded soups around the packet, wave and block sizes, the atrium;
* refitted with its own vertices a host tree keeps its Tri4 bytes and its boxes only grow;
* the refitted atrium tree is traced bit for bit like the oracle;
* any stream, reused pre-filled scratch: the same bytes;
* invalid arguments are refused on the host, invalid meshes and malformed hierarchies raise device flags.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import refit_wide_model as W
import test_refit_wide_model as T
from rodent_amd import formats as F
from rodent_amd import scene as S
from test_builder import write_obj

pytestmark = pytest.mark.gpu
WIDTHS = (4, 8)
BLOCK = {4: F.BVH4_TRI4, 8: F.BVH8_TRI4}
SOUPS = (1, 2, 3, 4, 5, 63, 64, 65, 256, 257, 1000, 100003)
cornell_scene = T.cornell_scene


@pytest.fixture(scope="module")
def gb(native_build):
    import torch
    from rodent_amd import gpubuild
    assert torch.cuda.is_available(), "these tests need a GPU"
    return gpubuild


@pytest.fixture(scope="module")
def atrium(native_build, tmp_path_factory):
    """(scene of the converter, {width: (nodes, tris)} of the host builder's .bvh)."""
    from rodent_amd import scenes
    path = scenes.scene_bvh("atrium")
    sc = S.convert(scenes.scene_obj("atrium"), tmp_path_factory.mktemp("atrium") / "atrium.rscene")
    return sc, {w: F.read_bvh(path, BLOCK[w]) for w in WIDTHS}


def plain_soup(n, seed):
    """n small triangles over 3n vertices, none degenerate (the host builder's spatial splits are not made for points and lines)."""
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), np.float32)
    v[:, :3] = (rng.uniform(-50, 50, (n, 1, 3)) + rng.uniform(-4, 4, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


@pytest.fixture(scope="module")
def soups(native_build, tmp_path_factory):
    """{n: (vertices, indices, {width: (nodes, tris)})}: the host builder's trees, one .bvh per soup."""
    d = tmp_path_factory.mktemp("soups")
    out = {}
    for n in SOUPS:
        v, ix = plain_soup(n, n)
        write_obj(d / "s.obj", v[:, :3], ix[:, :3])
        subprocess.run([native_build.BIN_DIR / "bvh_extractor", "-obj", d / "s.obj", "-o", d / "s.bvh"], check=True,
                       stdout=subprocess.DEVNULL, timeout=120)
        out[n] = (v, ix, {w: F.read_bvh(d / "s.bvh", BLOCK[w]) for w in WIDTHS})
    return out


def refit_equals_model(gb, width, nodes, tris, moved, ix, changed=True):
    """Refits on the device and in the model; asserts equal bytes and info.  Returns (DeviceBvh, model result)."""
    from rodent_amd import abi
    bvh = abi.DeviceBvh(width, nodes, tris, 0)
    model = W.refit(width, nodes, tris, moved, ix)
    assert gb.refit_wide(bvh, moved, ix) is bvh
    got = gb.download_wide(bvh)
    assert bvh.info.tolist() == model[2].tolist() == [len(nodes), int(W.valid_lanes(tris).sum()), 0, 0]
    assert got[0].tobytes() == model[0].tobytes()
    assert got[1].tobytes() == model[1].tobytes()
    if changed:
        assert got[0].tobytes() != nodes.tobytes() and got[1].tobytes() != tris.tobytes()
    return bvh, model


@pytest.mark.parametrize("width", WIDTHS)
def test_bytes_equal_the_model_after_a_deformation(gb, cornell, cornell_scene, soups, width):
    v, ix = cornell_scene.vertices, cornell_scene.indices
    refit_equals_model(gb, width, *cornell.blocks[width], W.deform(v, ix, seed=width), ix)
    for name, make in T.HAND_MADE.items():
        nodes, tris, v, ix = make(width)
        refit_equals_model(gb, width, nodes, tris, W.deform(v, ix, seed=5, collapse=1), ix)
    for n, (v, ix, blocks) in soups.items():
        nodes, tris = blocks[width]
        assert int(W.valid_lanes(tris).sum()) >= n
        refit_equals_model(gb, width, nodes, tris, W.deform(v, ix, seed=n, collapse=min(3, n - 1)), ix)


@pytest.mark.parametrize("width", WIDTHS)
def test_atrium_equals_the_model_and_its_own_vertices_keep_the_tri4_bytes(gb, atrium, cornell, cornell_scene, soups, width):
    sc, blocks = atrium
    refit_equals_model(gb, width, *blocks[width], W.deform(sc.vertices, sc.indices, seed=1), sc.indices)
    cases = [("atrium", sc.vertices, sc.indices, blocks[width]), ("cornell", cornell_scene.vertices, cornell_scene.indices,
                                                                   cornell.blocks[width]), ("soup", *soups[100003][:2], soups[100003][2][width])]
    for name, v, ix, (nodes, tris) in cases:
        bvh, _ = refit_equals_model(gb, width, nodes, tris, v, ix, changed=False)
        got = gb.download_wide(bvh)
        assert got[1].tobytes() == tris.tobytes(), name            # v0 / e1 / e2 / n: the host builder's own bytes
        assert W.contains(got[0], nodes).all(), name


@pytest.mark.parametrize("width", WIDTHS)
def test_traversal_of_the_refitted_atrium_is_bit_exact(gb, oracle, atrium, width):
    from rodent_amd import abi, raygen, scenes
    sc, blocks = atrium
    bvh = abi.DeviceBvh(width, *blocks[width], 0)
    moved = W.deform(sc.vertices, sc.indices, seed=1)
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    lo, hi = moved[:, :3].min(0), moved[:, :3].max(0)
    sets = {"primary": raygen.primary_rays(eye, d, up, fov, 256, 256, 0.0, scenes.PRIMARY_TMAX),
            "random": raygen.random_rays(lo, hi, 1 << 16, 7, 0.0, 1.0)}
    single = [v for v, name in enumerate(abi.variants(width)) if name == "single"][0]
    abi.top_min_rays(0)                           # every default launch through the persistent kernel that stages the top nodes
    try:
        first = {k: abi.traverse(bvh, rays, variant=0) for k, rays in sets.items()}
        gb.refit_wide(bvh, moved, sc.indices)
        nodes, tris = gb.download_wide(bvh)
        for k, rays in sets.items():
            for any_hit in (False, True):
                ref, st = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
                assert st["max_stack"] < 64
                for v in (0, single):
                    assert abi.traverse(bvh, rays, any_hit=any_hit, variant=v).tobytes() == ref.tobytes(), (k, any_hit, v)
                if not any_hit:
                    assert ref.tobytes() != first[k].tobytes(), k
    finally:
        abi.top_min_rays(-1)


@pytest.mark.parametrize("width", WIDTHS)
def test_deterministic_across_streams_and_reused_scratch(gb, soups, width):
    import torch
    from rodent_amd import abi
    v, ix, blocks = soups[100003]
    moved = W.deform(v, ix, seed=3)
    results = []
    big = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").fill_(0xAB)
    for stream, scratch in ((torch.cuda.Stream(), None), (torch.cuda.Stream(), None), (None, big), (None, big)):
        bvh = abi.DeviceBvh(width, *blocks[width], 0)
        gb.refit_wide(bvh, moved, ix, stream=stream, scratch=scratch)
        if scratch is not None:
            assert bvh.scratch is scratch
        results.append(tuple(x.tobytes() for x in gb.download_wide(bvh)))
    assert all(r == results[0] for r in results[1:])


@pytest.mark.parametrize("width", WIDTHS)
def test_refusals_and_flags(gb, width):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    sizes = l.rodent_hip_refit_wide_scratch_bytes
    assert sizes(width, 0, 1) == -1 and sizes(width, 1, 0) == -1 and sizes(2, 3, 7) == -1 and sizes(16, 3, 7) == -1
    assert sizes(width, 1, 1) > 0
    entry, entry_sync = (getattr(l, f"rodent_hip_refit_bvh{width}_tri4" + s) for s in ("", "_sync"))
    nodes, tris, v, ix = T.three_node_tree(width)
    nn, npk, n = len(nodes), len(tris), len(ix)
    good = abi.DeviceBvh(width, nodes, tris, 0)
    m_nodes, m_tris, m_info = W.refit(width, nodes, tris, v, ix)
    assert m_info.tolist() == [3, 17, 0, 0]
    # host-side refusals enqueue nothing: the hierarchy and the info words stay as they are
    vd, ixd = torch.from_numpy(v).cuda(), torch.from_numpy(ix).cuda()
    scratch = torch.empty(sizes(width, nn, npk), dtype=torch.uint8, device="cuda")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dev=0, nv=len(v), n=n, nn=nn, npk=npk, vp=vd.data_ptr(), ip=ixd.data_ptr(), nodes_p=good.nodes.data_ptr(),
             tris_p=good.tris.data_ptr(), sp=scratch.data_ptr(), fp=info.data_ptr()):
        return entry(dev, vp, nv, ip, n, nodes_p, nn, tris_p, npk, sp, fp, stream)
    assert call(n=0) == -1 and call(n=(1 << 25) + 1) == -1 and call(nv=0) == -3
    assert call(nn=0) == -11 and call(npk=0) == -11
    assert call(vp=None) == -4 and call(ip=None) == -4 and call(nodes_p=None) == -4 and call(tris_p=None) == -4 and call(sp=None) == -4
    assert call(fp=None) == -4 and call(dev=99) == -5
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [77] * 4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(good), (nodes, tris)))
    assert call() == 0
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [3, 17, 0, 0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(good), (m_nodes, m_tris)))
    # the sync form, on device pointers too
    host_info = (C.c_int32 * 4)()
    assert entry_sync(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, good.nodes.data_ptr(), nn, good.tris.data_ptr(), npk, host_info) == 0
    assert list(host_info) == [3, 17, 0, 0]
    assert entry_sync(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, good.nodes.data_ptr(), 0, good.tris.data_ptr(), npk, host_info) == -11
    # an index outside the vertex array (spare rows behind `nv`: a missing guard would still read inside the buffer), a NaN
    bad = ix.copy(); bad[5, 1] = len(v)
    spare = torch.from_numpy(np.concatenate([v, np.ones((8, 4), np.float32)])).cuda()
    bad_d = torch.from_numpy(bad).cuda()
    b = abi.DeviceBvh(width, nodes, tris, 0)
    assert call(vp=spare.data_ptr(), ip=bad_d.data_ptr(), nodes_p=b.nodes.data_ptr(), tris_p=b.tris.data_ptr()) == 0
    model = W.refit(width, nodes, tris, v, bad)
    assert info.cpu().tolist() == model[2].tolist() == [3, 17, gb.BAD_INDEX, 0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gb.download_wide(b), model[:2]))       # the vertex read as the origin
    with pytest.raises(gb.BuildError, match="index"):
        gb.refit_wide(abi.DeviceBvh(width, nodes, tris, 0), v, bad)
    nan = v.copy(); nan[4, 1] = np.nan
    b = abi.DeviceBvh(width, nodes, tris, 0)
    with pytest.raises(gb.BuildError, match="non-finite"):
        gb.refit_wide(b, nan, ix)
    assert b.info.tolist() == W.refit(width, nodes, tris, nan, ix)[2].tolist() == [3, 17, gb.NON_FINITE, 0]
    # malformed trees: the flag and the completed count of the model; every word the rules do not name stays
    for name, (m_n, m_t, m_v, m_ix, want) in T.malformed(width).items():
        b = abi.DeviceBvh(width, m_n, m_t, 0)
        with pytest.raises(gb.BuildError, match="malformed"):
            gb.refit_wide(b, m_v, m_ix)
        model = W.refit(width, m_n, m_t, m_v, m_ix)
        assert b.info.tolist() == model[2].tolist() == want, name
        got = gb.download_wide(b)
        T.assert_only_the_rules_words_change((m_n, m_t), got)
        assert got[1].tobytes() == model[1].tobytes(), name
        assert got[0].tobytes() == model[0].tobytes(), name        # both claims of a node come from one thread, in slot order
        assert entry_sync(0, vd.data_ptr(), len(v), ixd.data_ptr(), n, b.nodes.data_ptr(), nn, b.tris.data_ptr(), npk, host_info) == -7
        assert host_info[2] == gb.BAD_TOPOLOGY
    with pytest.raises(ValueError):
        gb.refit_wide(abi.DeviceBvh(2, np.zeros(1, F.NODE2), np.zeros(1, F.TRI1), 0), v, ix)
    # a clean refit afterwards: the flags are per call
    assert gb.refit_wide(abi.DeviceBvh(width, nodes, tris, 0), v, ix).info.tolist() == [3, 17, 0, 0]
