"""The device collapse under a stack limit (rodent_hip_collapse_bvh2_tri1_bounded, csrc/build_collapse.h; gpubuild.collapse_wide and
build_wide with stack_limit) on the GPU.

* nodes, packets and info words equal tests/collapse_bounded_model.py's byte for byte: every fixture of test_collapse_bounded_model.py at
  every limit it uses, a 100 003-triangle LBVH at L = 24 and 63, a pre-split tree; the input is only read;
* L = 0 through the bounded entry gives the bytes of the entry without a limit;
* the same bytes on any stream and into reused pre-filled scratch;
* a bushy spine over a soup, collapsed with L = 63 and with L = H(0) = 43, is traced without asking the oracle first -- info[3] <= 63
  is the guarantee -- and the hit records equal the oracle's bit for bit;
* the tool's --stack-limit writes the model's bytes.
"""
import ctypes as C

import numpy as np
import pytest

import collapse_bounded_model as BM
import collapse_model as M
import test_collapse_bounded_model as TB
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
def all_cases():
    return TB.cases()


@pytest.fixture(scope="module")
def big(gb):
    """A 100 003-triangle soup's device LBVH (max_leaf 4), downloaded."""
    v, ix = T.soup(100003, 7)
    return gb.download(gb.build_bvh2(v, ix, 4))


def collapse_equals_model(gb, width, L, nodes, tris, model=None, **kw):
    """Collapses on the device and in the model; asserts equal bytes and info, and that the input is only read.  Returns the DeviceBvh."""
    from rodent_amd import abi
    bvh2 = abi.DeviceBvh(2, nodes, tris, 0)
    model = BM.collapse(width, nodes, tris, L) if model is None else model
    wide = gb.collapse_wide(bvh2, width, stack_limit=L, **kw)
    assert wide.width == width and wide.info.tolist() == model[2].tolist() and model[2][2] == 0
    assert (wide.num_nodes, wide.num_tris) == (len(model[0]), len(model[1]))
    got = gb.download_wide(wide)
    assert got[0].tobytes() == model[0].tobytes()
    assert got[1].tobytes() == model[1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(bvh2), (nodes, tris)))      # the input is only read
    return wide


@pytest.mark.parametrize("width", WIDTHS)
def test_bytes_equal_the_model_on_every_fixture(gb, all_cases, width):
    changed = 0
    for c in all_cases:
        for L in c.limits(width):
            try:
                collapse_equals_model(gb, width, L, c.nodes, c.tris, c.bounded(width, L))
            except AssertionError as e:
                raise AssertionError(f"{c.name}, L = {L}") from e
            changed += not TB.same(c.bounded(width, L), c.unbounded[width])
    assert changed > 0                                            # the limit was at work


@pytest.mark.parametrize("width", WIDTHS)
def test_bytes_equal_the_model_on_large_and_split_trees(gb, big, width):
    free = M.collapse(width, *big)
    changed = 0
    for L in (24, 63):
        model = BM.collapse(width, *big, L)
        wide = collapse_equals_model(gb, width, L, *big, model)
        print(f"width {width} L {L}: B {wide.info[3]} (no limit: {free[2][3]}), wide nodes {wide.num_nodes} (no limit: {len(free[0])})")
        changed += not TB.same(model, free)
    assert changed > 0
    # a pre-split tree: references, several records to a triangle
    v, ix = T.soup(1000, 5)
    split = gb.build_bvh2(v, ix, 4, treelet_passes=3, split_budget=1.0)
    assert split.num_tris > 1000
    nodes, tris = gb.download(split)
    for L in (12, 63):
        collapse_equals_model(gb, width, L, nodes, tris)
    # build_wide passes the limit on
    wide = gb.build_wide(v, ix, width, max_leaf=4, stack_limit=12)
    model = BM.collapse(width, *gb.download(wide.bvh2), 12)
    assert wide.info.tolist() == model[2].tolist()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(wide), model[:2]))


@pytest.mark.parametrize("width", WIDTHS)
def test_no_limit_through_the_bounded_entry_is_the_old_entry(gb, big, width):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    node_dt = M.NODE[width]
    for nodes, tris in (big, TB.bushy_spine(40, 8), T.sound_hand_tree()):
        bvh2 = abi.DeviceBvh(2, nodes, tris, 0)
        nn, nt = len(nodes), len(tris)
        old = gb.collapse_wide(bvh2, width)
        wide_d = torch.full((nn * node_dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        pk_d = torch.full((nt * F.TRI4.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        scratch = torch.full((l.rodent_hip_collapse_bounded_scratch_bytes(width, nn, nt),), 0xAB, dtype=torch.uint8, device="cuda")
        info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(limit, dev=0, w=width):
            return l.rodent_hip_collapse_bvh2_tri1_bounded(dev, w, limit, bvh2.nodes.data_ptr(), nn, bvh2.tris.data_ptr(), nt,
                                                           wide_d.data_ptr(), pk_d.data_ptr(), scratch.data_ptr(), info.data_ptr(), stream)
        # refusals enqueue nothing
        assert call(64) == -13 and call(-1) == -13 and call(63, w=3) == -12 and call(63, dev=99) == -5
        torch.cuda.synchronize()
        assert info.cpu().tolist() == [77] * 4 and (wide_d == 0x5A).all().item() and (pk_d == 0x5A).all().item()
        assert call(0) == 0
        torch.cuda.synchronize()
        assert info.cpu().tolist() == old.info.tolist()
        want = gb.download_wide(old)
        assert wide_d[: old.num_nodes * node_dt.itemsize].cpu().numpy().tobytes() == want[0].tobytes()
        assert pk_d[: old.num_tris * F.TRI4.itemsize].cpu().numpy().tobytes() == want[1].tobytes()
        # the sync form, with a limit
        host = (C.c_int32 * 4)()
        sync = l.rodent_hip_collapse_bvh2_tri1_bounded_sync
        assert sync(0, width, 63, bvh2.nodes.data_ptr(), nn, bvh2.tris.data_ptr(), nt, wide_d.data_ptr(), pk_d.data_ptr(), host) == 0
        assert list(host) == gb.collapse_wide(bvh2, width, stack_limit=63).info.tolist()
    with pytest.raises(gb.BuildError, match="stack_limit"):
        gb.collapse_wide(bvh2, width, stack_limit=64)
    with pytest.raises(gb.BuildError, match="stack_limit"):
        gb.build_wide(*T.soup(10, 1), width, stack_limit=-1)
    # a malformed tree raises the flag under a limit too
    bad = abi.DeviceBvh(2, *T.malformed()["a node named by two slots"], 0)
    with pytest.raises(gb.BuildError, match="malformed"):
        gb.collapse_wide(bad, width, stack_limit=63)


@pytest.mark.parametrize("width", WIDTHS)
def test_deterministic_across_streams_and_reused_scratch(gb, big, width):
    import torch
    from rodent_amd import abi
    for (nodes, tris), L in ((big, 24), (TB.bushy_spine(40, 8), 63)):
        results = []
        filled = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").fill_(0xAB)
        for stream, scratch in ((torch.cuda.Stream(), None), (torch.cuda.Stream(), None), (None, filled), (None, filled)):
            wide = gb.collapse_wide(abi.DeviceBvh(2, nodes, tris, 0), width, stream=stream, scratch=scratch, stack_limit=L)
            if scratch is not None:
                assert wide.scratch is scratch
            results.append((wide.info.tobytes(), *(x.tobytes() for x in gb.download_wide(wide))))
        assert all(r == results[0] for r in results[1:])
        model = BM.collapse(width, nodes, tris, L)
        assert results[0] == (model[2].tobytes(), model[0].tobytes(), model[1].tobytes())


@pytest.fixture(scope="module")
def deep(oracle):
    """A bushy spine over a plain soup, 16 Ki random rays, and what the oracle finds on the BVH2."""
    from rodent_amd import raygen
    v, ix, nodes, tris = TB.spine_over_soup(40, 8, 40)
    rays = raygen.random_rays(v[:, :3].min(0), v[:, :3].max(0), 1 << 14, 3, 0.0, 1.0)
    return nodes, tris, rays, oracle.traverse(2, nodes, tris, rays)[0]


@pytest.mark.parametrize("width", WIDTHS)
def test_a_deep_tree_collapsed_under_63_is_traced_like_the_oracle(gb, oracle, deep, width):
    from rodent_amd import abi
    nodes, tris, rays, on_bvh2 = deep
    small = TB.small_flags(nodes, tris)
    assert TB.height_of_input(nodes, small) == 43
    bvh2_ids = abi.traverse(abi.DeviceBvh(2, nodes, tris, 0), rays, variant=0)["tri_id"]
    assert np.array_equal(bvh2_ids, on_bvh2["tri_id"])
    free = M.collapse(width, nodes, tris)
    for L in (63, 43):                                            # the limit of the kernels' stack, and H(0): the tightest that can be met
        wide = collapse_equals_model(gb, width, L, nodes, tris)
        print(f"width {width}: B {wide.info[3]} under L = {L}, {free[2][3]} without a limit")
        out, pk = gb.download_wide(wide)
        for any_hit in (False, True):
            ref, st = oracle.traverse(width, out, pk, rays, any_hit=any_hit, algo="gpu")
            assert st["max_stack"] - 1 <= wide.info[3] <= L
            assert abi.traverse(wide, rays, any_hit=any_hit, variant=0).tobytes() == ref.tobytes(), (L, any_hit)
            assert (ref["tri_id"] >= 0).any()
        # the same triangles as tracing the BVH2
        assert np.array_equal(abi.traverse(wide, rays, variant=0)["tri_id"], bvh2_ids), L
    assert free[2][3] > 43                                        # H(0) as the limit changed the tree


def test_the_tool_writes_the_bounded_wide_block(gb, native_build, tmp_path):
    from conftest import GOLDEN
    from rodent_amd import abi
    sc = S.convert(GOLDEN / "cornell_box.obj", tmp_path / "cornell.rscene")
    gb.main([str(tmp_path / "cornell.rscene"), "-o", str(tmp_path / "out.bvh"), "--max-leaf", "1", "--width", "8", "--stack-limit", "63"])
    nodes, tris = F.read_bvh(tmp_path / "out.bvh", F.BVH2_TRI1)
    assert len(tris) == sc.num_tris
    got = F.read_bvh(tmp_path / "out.bvh", abi.BLOCK_OF_WIDTH[8])
    model = BM.collapse(8, nodes, tris, 63)
    assert got[0].tobytes() == model[0].tobytes() and got[1].tobytes() == model[1].tobytes()
    # a limit that bites on this tree: other bytes than without one, the model's again
    small = TB.small_flags(nodes, tris)
    tight = TB.height_of_input(nodes, small)
    gb.main([str(tmp_path / "cornell.rscene"), "-o", str(tmp_path / "tight.bvh"), "--max-leaf", "1", "--width", "8", "--stack-limit", str(tight)])
    got = F.read_bvh(tmp_path / "tight.bvh", abi.BLOCK_OF_WIDTH[8])
    model = BM.collapse(8, nodes, tris, tight)
    assert got[0].tobytes() == model[0].tobytes() and got[1].tobytes() == model[1].tobytes()
    assert TB.bound_of_output(got[0]) <= tight
