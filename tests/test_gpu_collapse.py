"""The device collapse of BVH2 / Tri1 into BVH4 / BVH8 + Tri4 (rodent_hip_collapse_bvh2_tri1, csrc/build_collapse.h; gpubuild.collapse_wide
and build_wide) on the GPU.

* nodes, packets and info words equal tests/collapse_model.py's byte for byte: Cornell's host tree, the soup trees of
  test_collapse_model.py (LBVH and 3 treelet passes), a 100 003-triangle LBVH, a pre-split tree, the atrium; on any stream, into
  reused pre-filled scratch;
* collapse then refit equals the two models one after the other, and with its own vertices an unsplit tree keeps every byte;
* collapsed trees are traced bit for bit like the oracle -- after the oracle has shown, on the CPU, that no stack passes 64 entries;
* malformed trees raise the flag, invalid arguments are refused on the host with nothing enqueued.
"""
import ctypes as C

import numpy as np
import pytest

import collapse_model as M
import refit_wide_model as W
import test_collapse_model as T
from rodent_amd import formats as F
from rodent_amd import scene as S

pytestmark = pytest.mark.gpu
WIDTHS = (4, 8)


@pytest.fixture(scope="module")
def gb(native_build):
    import torch
    from rodent_amd import gpubuild
    assert torch.cuda.is_available(), "these tests need a GPU"
    return gpubuild


@pytest.fixture(scope="module")
def atrium(native_build, tmp_path_factory):
    from rodent_amd import scenes
    return S.convert(scenes.scene_obj("atrium"), tmp_path_factory.mktemp("atrium") / "atrium.rscene")


@pytest.fixture(scope="module")
def trees():
    return list(T.soup_trees())


@pytest.fixture(scope="module")
def big(gb):
    """A 100 003-triangle soup and its device LBVH (max_leaf 4), downloaded."""
    v, ix = T.soup(100003, 7)
    return v, ix, gb.download(gb.build_bvh2(v, ix, 4))


def collapse_equals_model(gb, width, nodes, tris, **kw):
    """Collapses on the device and in the model; asserts equal bytes and info.  Returns (wide DeviceBvh, model result)."""
    from rodent_amd import abi
    bvh2 = abi.DeviceBvh(2, nodes, tris, 0)
    model = M.collapse(width, nodes, tris)
    wide = gb.collapse_wide(bvh2, width, **kw)
    assert wide.width == width and wide.info.tolist() == model[2].tolist() and model[2][2] == 0
    assert (wide.num_nodes, wide.num_tris) == (len(model[0]), len(model[1]))
    got = gb.download_wide(wide)
    assert got[0].tobytes() == model[0].tobytes()
    assert got[1].tobytes() == model[1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(bvh2), (nodes, tris)))      # the input is only read
    return wide, model


@pytest.mark.parametrize("width", WIDTHS)
def test_bytes_equal_the_model(gb, trees, big, width):
    collapse_equals_model(gb, width, *T.golden_cornell())
    for name, _, _, nodes, tris in trees:
        collapse_equals_model(gb, width, nodes, tris)
    wide, model = collapse_equals_model(gb, width, *big[2])
    assert model[2][1] < len(big[2][1]) and model[2][0] < len(big[2][0])
    # a pre-split tree: references, several records to a triangle
    v, ix = T.soup(1000, 5)
    split = gb.build_bvh2(v, ix, 4, treelet_passes=3, split_budget=1.0)
    assert split.num_tris > 1000
    collapse_equals_model(gb, width, *gb.download(split))
    prims = list(range(64)); prims[63] |= T.INT_MIN                # a run of 64 records, the longest
    collapse_equals_model(gb, width, *T.hand_tree([[~0, ~64]], prims + [T.INT_MIN | np.int32(64)]))
    collapse_equals_model(gb, width, *T.sound_hand_tree())
    collapse_equals_model(gb, width, *T.deep_chain(65))


@pytest.mark.parametrize("width", WIDTHS)
def test_atrium_build_wide_equals_the_models_and_is_traced_like_the_oracle(gb, oracle, atrium, width):
    from rodent_amd import abi, raygen, scenes
    wide = gb.build_wide(atrium.vertices, atrium.indices, width, max_leaf=4, treelet_passes=3)
    assert wide.bvh2.width == 2 and wide.bvh2.num_tris == atrium.num_tris
    nodes, tris = gb.download(wide.bvh2)
    model = M.collapse(width, nodes, tris)
    got = gb.download_wide(wide)
    assert wide.info.tolist() == model[2].tolist()
    assert got[0].tobytes() == model[0].tobytes() and got[1].tobytes() == model[1].tobytes()
    T.assert_structure(width, nodes, tris, *got, wide.info)
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    lo, hi = atrium.vertices[:, :3].min(0), atrium.vertices[:, :3].max(0)
    sets = {"primary": raygen.primary_rays(eye, d, up, fov, 128, 128, 0.0, scenes.PRIMARY_TMAX),
            "random": raygen.random_rays(lo, hi, 1 << 14, 7, 0.0, 1.0)}
    trace_like_the_oracle(oracle, wide, model, sets)


def trace_like_the_oracle(oracle, wide, model, sets):
    """The oracle first, on the CPU, over the model's tree: only rays whose stacks it has shown to fit are sent to the device."""
    from rodent_amd import abi
    for k, rays in sets.items():
        for any_hit in (False, True):
            ref, st = oracle.traverse(wide.width, model[0], model[1], rays, any_hit=any_hit, algo="gpu")
            print(f"width {wide.width} {k} any_hit {any_hit}: max_stack {st['max_stack']}, B {model[2][3]}")
            assert st["max_stack"] <= 64 and st["max_stack"] - 1 <= model[2][3]
            assert abi.traverse(wide, rays, any_hit=any_hit, variant=0).tobytes() == ref.tobytes(), (k, any_hit)
            assert (ref["tri_id"] >= 0).any(), k


@pytest.mark.parametrize("width", WIDTHS)
def test_cornell_and_a_soup_are_traced_like_the_oracle(gb, oracle, cornell, width):
    from rodent_amd import abi, raygen
    wide, model = collapse_equals_model(gb, width, *T.golden_cornell())
    trace_like_the_oracle(oracle, wide, model, {k: cornell.ray_sets[k] for k in sorted(cornell.ray_sets)})
    v, ix = T.plain_soup(1000, 1000)
    for options in (dict(max_leaf=4), dict(max_leaf=4, treelet_passes=3)):
        wide = gb.build_wide(v, ix, width, **options)
        nodes, tris = gb.download(wide.bvh2)
        model = M.collapse(width, nodes, tris)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(wide), model[:2]))
        rays = raygen.random_rays(v[:, :3].min(0), v[:, :3].max(0), 1 << 14, 3, 0.0, 1.0)
        trace_like_the_oracle(oracle, wide, model, {"random": rays})
        # the same triangles as on the BVH2 it came from
        assert np.array_equal(abi.traverse(wide, rays, variant=0)["tri_id"], abi.traverse(wide.bvh2, rays, variant=0)["tri_id"])


@pytest.mark.parametrize("width", WIDTHS)
def test_deterministic_across_streams_and_reused_scratch(gb, big, width):
    import torch
    from rodent_amd import abi
    nodes, tris = big[2]
    results = []
    filled = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").fill_(0xAB)
    for stream, scratch in ((torch.cuda.Stream(), None), (torch.cuda.Stream(), None), (None, filled), (None, filled)):
        wide = gb.collapse_wide(abi.DeviceBvh(2, nodes, tris, 0), width, stream=stream, scratch=scratch)
        if scratch is not None:
            assert wide.scratch is scratch
        results.append((wide.info.tobytes(), *(x.tobytes() for x in gb.download_wide(wide))))
    assert all(r == results[0] for r in results[1:])
    model = M.collapse(width, nodes, tris)
    assert results[0] == (model[2].tobytes(), model[0].tobytes(), model[1].tobytes())


@pytest.mark.parametrize("width", WIDTHS)
def test_collapse_then_refit_equals_the_model_chain(gb, trees, big, width):
    cases = [(name, v, ix, nodes, tris) for name, v, ix, nodes, tris in trees if name.split("-")[1] in ("5", "65", "1000")]
    cases.append(("big", big[0], big[1], *big[2]))
    for name, v, ix, nodes, tris in cases:
        n = len(ix)
        wide, model = collapse_equals_model(gb, width, nodes, tris)
        # its own vertices: every byte stays (an unsplit device tree's boxes are exact unions)
        gb.refit_wide(wide, v, ix)
        assert wide.info.tolist() == [len(model[0]), len(tris), 0, 0], name
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(wide), model[:2])), name
        moved = W.deform(v, ix, seed=n, collapse=min(3, n - 1))
        chain = W.refit(width, model[0], model[1], moved, ix)
        gb.refit_wide(wide, moved, ix)
        assert wide.info.tolist() == chain[2].tolist(), name
        got = gb.download_wide(wide)
        assert got[0].tobytes() == chain[0].tobytes() and got[1].tobytes() == chain[1].tobytes(), name
        assert got[0].tobytes() != model[0].tobytes() or n < 3, name


@pytest.mark.parametrize("width", WIDTHS)
def test_refusals_and_flags(gb, width):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    nodes, tris = T.sound_hand_tree()
    nn, nt = len(nodes), len(tris)
    model = M.collapse(width, nodes, tris)
    bvh2 = abi.DeviceBvh(2, nodes, tris, 0)
    node_dt = M.NODE[width]
    wide_d = torch.full((nn * node_dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    pk_d = torch.full((nt * F.TRI4.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(l.rodent_hip_collapse_scratch_bytes(width, nn, nt), dtype=torch.uint8, device="cuda")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dev=0, width=width, nodes_p=bvh2.nodes.data_ptr(), nn=nn, tris_p=bvh2.tris.data_ptr(), nt=nt, wp=wide_d.data_ptr(),
             pp=pk_d.data_ptr(), sp=scratch.data_ptr(), fp=info.data_ptr()):
        return l.rodent_hip_collapse_bvh2_tri1(dev, width, nodes_p, nn, tris_p, nt, wp, pp, sp, fp, stream)
    # host-side refusals enqueue nothing: the outputs and the info words stay as they are
    assert call(width=3) == -12 and call(width=2) == -12 and call(width=16) == -12
    assert call(nn=0) == -11 and call(nt=0) == -11
    assert call(nodes_p=None) == -4 and call(tris_p=None) == -4 and call(wp=None) == -4 and call(pp=None) == -4
    assert call(sp=None) == -4 and call(fp=None) == -4 and call(dev=99) == -5
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [77] * 4
    assert (wide_d == 0x5A).all().item() and (pk_d == 0x5A).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert info.cpu().tolist() == model[2].tolist()
    W_, P_ = int(model[2][0]), int(model[2][1])
    assert wide_d[: W_ * node_dt.itemsize].cpu().numpy().tobytes() == model[0].tobytes()
    assert pk_d[: P_ * F.TRI4.itemsize].cpu().numpy().tobytes() == model[1].tobytes()
    # the sync form, on device pointers too
    host = (C.c_int32 * 4)()
    sync = l.rodent_hip_collapse_bvh2_tri1_sync
    assert sync(0, width, bvh2.nodes.data_ptr(), nn, bvh2.tris.data_ptr(), nt, wide_d.data_ptr(), pk_d.data_ptr(), host) == 0
    assert list(host) == model[2].tolist()
    assert sync(0, 5, bvh2.nodes.data_ptr(), nn, bvh2.tris.data_ptr(), nt, wide_d.data_ptr(), pk_d.data_ptr(), host) == -12
    assert sync(0, width, bvh2.nodes.data_ptr(), 0, bvh2.tris.data_ptr(), nt, wide_d.data_ptr(), pk_d.data_ptr(), host) == -11
    # malformed trees: the flag, in both forms; the process goes on
    for name, (m_n, m_t) in T.malformed().items():
        assert M.collapse(width, m_n, m_t)[2][2] == gb.BAD_TOPOLOGY, name
        bad = abi.DeviceBvh(2, m_n, m_t, 0)
        with pytest.raises(gb.BuildError, match="malformed"):
            gb.collapse_wide(bad, width)
        big_w = torch.empty(len(m_n) * node_dt.itemsize, dtype=torch.uint8, device="cuda")
        big_p = torch.empty(len(m_t) * F.TRI4.itemsize, dtype=torch.uint8, device="cuda")
        rc = sync(0, width, bad.nodes.data_ptr(), len(m_n), bad.tris.data_ptr(), len(m_t), big_w.data_ptr(), big_p.data_ptr(), host)
        assert rc == -7 and host[2] == gb.BAD_TOPOLOGY, name
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(bad), (m_n, m_t))), name
    with pytest.raises(ValueError):
        gb.collapse_wide(abi.DeviceBvh(4, np.zeros(1, F.NODE4), np.zeros(1, F.TRI4), 0), width)
    with pytest.raises(gb.BuildError, match="width"):
        gb.collapse_wide(bvh2, 3)
    # a clean collapse afterwards: the flags are per call
    assert gb.collapse_wide(bvh2, width).info.tolist() == model[2].tolist()


def test_the_tool_writes_the_wide_blocks(gb, native_build, tmp_path):
    from conftest import GOLDEN
    from rodent_amd import abi
    sc = S.convert(GOLDEN / "cornell_box.obj", tmp_path / "cornell.rscene")
    gb.main([str(tmp_path / "cornell.rscene"), "-o", str(tmp_path / "out.bvh"), "--max-leaf", "4", "--width", "4", "--width", "8"])
    nodes, tris = F.read_bvh(tmp_path / "out.bvh", F.BVH2_TRI1)
    assert len(tris) == sc.num_tris
    for width in WIDTHS:
        got = F.read_bvh(tmp_path / "out.bvh", abi.BLOCK_OF_WIDTH[width])
        model = M.collapse(width, nodes, tris)
        assert got[0].tobytes() == model[0].tobytes() and got[1].tobytes() == model[1].tobytes()
