"""CPU tests of the deep BVH4 / BVH8 fixture (wide_fixtures.chain_wide): the stack depth it promises, the oracle's hits on it
against an independent float64 Moeller-Trumbore, and the two oracle orders against each other.  The GPU tests that use the fixture
are in test_gpu_wide_edges.py."""
import numpy as np
import pytest

import wide_fixtures as W
from conftest import ambiguous_mask
from test_oracle import mt_float64


def rays_1000():
    """The rays of test_deep_stack_falls_back_to_global_stack: 1000 along (0.001, 0.002, 1), every third misses."""
    return W.chain_rays(1000, 0)


@pytest.mark.parametrize("arity", [4, 8])
@pytest.mark.parametrize("fan", [1, 3, "arity-1"])
@pytest.mark.parametrize("any_hit", [False, True])
def test_stack_peak_is_what_the_construction_promises(oracle, arity, fan, any_hit):
    fan = arity - 1 if fan == "arity-1" else fan
    rays = rays_1000()
    for depth in (1, 2, 5, 63 // fan):
        for last_fan in (None, 1, fan):
            nodes, tris = W.chain_wide(arity, depth, fan, chain_last=any_hit, last_fan=last_fan)
            leaves, nz, peak = W.chain_counts(depth, fan, last_fan)
            assert len(tris) == leaves == nz and peak == sum(W.level_fans(depth, fan, last_fan))
            hits, st = oracle.traverse(arity, nodes, tris, rays, any_hit=any_hit, algo="gpu")
            assert st["max_stack"] == peak + 1, (depth, last_fan)           # the wide oracle counts the sentinel
            assert (hits["tri_id"] >= 0).sum() > 600 and (hits["tri_id"][::3] == -1).all()
            if not any_hit:
                assert set(hits["tri_id"][hits["tri_id"] >= 0]) == {0}      # every triangle accepted on the way to triangle 0
    if any_hit:
        # with the chain in slot 0 an occlusion ray pushes the chain under the leaves and ends on the root's first leaf
        nodes, tris = W.chain_wide(arity, 40 // fan, fan, chain_last=False)
        assert oracle.traverse(arity, nodes, tris, rays, any_hit=True, algo="gpu")[1]["max_stack"] == fan + 1


@pytest.mark.parametrize("arity", [4, 8])
@pytest.mark.parametrize("any_hit", [False, True])
def test_capacity_is_63_entries(oracle, arity, any_hit):
    """64 slots, one of them the sentinel (stack.impala:53-54; `ptr + 1 >= STACK_CAP` in traverse_gpu_wide): 62 and 63 entries
    trace, 64 raise -- with one leaf per level and with arity - 1 leaves per level (a node step that would cross the end)."""
    rays = rays_1000()
    for fan in (1, arity - 1):
        for peak in (62, 63):
            (nodes, tris), _ = W.chain_wide_peak(arity, peak, fan, chain_last=any_hit)
            assert oracle.traverse(arity, nodes, tris, rays, any_hit=any_hit, algo="gpu")[1]["max_stack"] == peak + 1
        (nodes, tris), _ = W.chain_wide_peak(arity, 64, fan, chain_last=any_hit)
        with pytest.raises(RuntimeError, match="stack overflow"):
            oracle.traverse(arity, nodes, tris, rays, any_hit=any_hit, algo="gpu")


@pytest.mark.parametrize("arity", [4, 8])
def test_miss_every_leaves_the_deepest_triangle_out(oracle, arity):
    """miss_every: the boxes stay, so the stack is as deep; an any-hit ray pops entries from the far end until it meets a triangle
    that is still in its way, which is not the deepest one."""
    rays = rays_1000()
    for fan in (1, arity - 1):
        depth = 40 // fan
        k = W.miss_every_for(depth, fan)
        nodes, tris = W.chain_wide(arity, depth, fan, chain_last=True, miss_every=k)
        leaves, nz, peak = W.chain_counts(depth, fan)
        hits, st = oracle.traverse(arity, nodes, tris, rays, any_hit=True, algo="gpu")
        assert st["max_stack"] == peak + 1
        found = set(hits["tri_id"][hits["tri_id"] >= 0])
        assert len(found) == 1 and 0 <= min(found) < leaves - 1 and min(found) % k == 0
        closest, st = oracle.traverse(arity, nodes, tris, rays, algo="gpu")
        assert st["max_stack"] == peak + 1 and set(closest["tri_id"][closest["tri_id"] >= 0]) == {0}


@pytest.mark.parametrize("arity", [4, 8])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("chain_last", [False, True])
def test_closest_hits_equal_float64_moeller_trumbore(oracle, arity, ties, chain_last):
    fan = arity - 1
    rays = W.chain_rays(1000, 1, jitter=True, cut=(W.Z0 - 5, W.Z0 + 45))
    depth = 60 // fan
    k = W.miss_every_for(depth, fan, None, ties)
    for miss_every in (0, k):
        nodes, tris = W.chain_wide(arity, depth, fan, chain_last=chain_last, miss_every=miss_every, ties=ties)
        hits, _ = oracle.traverse(arity, nodes, tris, rays, algo="gpu")
        flat, ids = W.flatten_tri4(tris)
        assert len(flat) == len(tris) and np.array_equal(ids, np.arange(len(tris)))
        t64 = mt_float64(flat, rays)
        hit = hits["tri_id"] >= 0
        assert np.array_equal(hit, np.isfinite(t64))            # big triangles hit well inside: no grazing rays here
        assert 300 < hit.sum() < len(rays) - 300
        assert np.allclose(hits["t"][hit], t64[hit], rtol=1e-5, atol=0)
        assert np.array_equal(hits["t"][~hit], rays["tmax"][~hit])
        brute, second = oracle.brute_force(tris, rays)
        amb = ambiguous_mask(brute, second)
        assert np.array_equal(brute["tri_id"] >= 0, hit)
        assert np.array_equal(hits["tri_id"][~amb], brute["tri_id"][~amb])
        if ties:
            assert amb[hit].mean() >= 0.10                      # otherwise the fixture does not test what it claims
            # ... and whichever duplicate the visit order picks, it lies at the same distance
            assert np.array_equal(hits["t"][amb], brute["t"][amb])
        else:
            assert not amb.any()


@pytest.mark.parametrize("arity", [4, 8])
@pytest.mark.parametrize("any_hit", [False, True])
def test_cpu_order_and_gpu_order_oracles_agree(oracle, arity, any_hit):
    """algo="ref" (the CPU kernel's sorted order, culling on pop) and algo="gpu" visit the chain differently but must agree on
    hit / miss and on t (closest hit; an any-hit ray may stop at another occluder)."""
    rays = W.chain_rays(1000, 2, jitter=True, cut=(W.Z0 - 5, W.Z0 + 70))
    for fan in (1, arity - 1):
        for ties in ((False, True) if fan > 1 else (False,)):
            depth = 60 // fan
            for miss_every in (0, W.miss_every_for(depth, fan, None, ties)):
                nodes, tris = W.chain_wide(arity, depth, fan, chain_last=any_hit, miss_every=miss_every, ties=ties)
                ref, _ = oracle.traverse(arity, nodes, tris, rays, any_hit=any_hit, algo="ref")
                gpu, _ = oracle.traverse(arity, nodes, tris, rays, any_hit=any_hit, algo="gpu")
                assert np.array_equal(ref["tri_id"] >= 0, gpu["tri_id"] >= 0)
                if not any_hit:
                    assert ref["t"].tobytes() == gpu["t"].tobytes()


def test_ray_peaks_counts_real_entries(oracle):
    (nodes, tris), _ = W.chain_wide_peak(8, 25, 7)
    rays = W.chain_rays(300, 3, cut=(W.Z0 - 5, W.Z0 + 30))
    peaks = W.ray_peaks(oracle, 8, nodes, tris, rays)
    assert peaks.max() == 25 and (peaks[::3] == -1).all()       # a ray that misses the root's boxes pushes nothing
    assert len(set(peaks)) > 5                                  # the cut rays stop at different depths
