"""The BVH4 / BVH8 kernels (rodent_amd/csrc/traversal_wide.h) where their stack leaves the LDS window, and at edge rays.

A wide lane's stack is an LDS-only window of LDS_N rows (16 / 24).  A node step that leaves the top of the stack at row >= LDS_N
abandons the ray: its id goes to the launch's deep list and k_wide_finish, the second kernel of every launch, traces it again from
the root with wide_ray_literal -- a separately written loop -- on a 64-entry stack, and stores its record on top of whatever the
first kernel stored.  Everything here is compared with oracle.traverse(width, ..., algo="gpu") as bytes, for every order-preserving
mapping, through the persistent form (rodent_hip_top_min_rays(0)) and with the shipped threshold (the one-chunk kernel at these
sizes).  The trees come from wide_fixtures.chain_wide, whose stack depth test_wide_fixtures.py pins on the CPU."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import wide_fixtures as W
from rodent_amd import formats as F

pytestmark = pytest.mark.gpu

WIDTHS = (4, 8)
FORMS = (0, -1)                # rodent_hip_top_min_rays: 0 = k_wide_top_persist at every size, -1 = the shipped threshold


@pytest.fixture(scope="module")
def gpu(native_build):
    import torch
    from rodent_amd import abi
    assert torch.cuda.is_available(), "these tests need a GPU"
    t0 = time.perf_counter()
    yield abi
    abi.lib().rodent_hip_top_min_rays(-1)
    print(f"\ntest_gpu_wide_edges.py: {time.perf_counter() - t0:.1f} s wall")


@contextlib.contextmanager
def form(gpu, min_rays):
    gpu.lib().rodent_hip_top_min_rays(min_rays)
    try:
        yield
    finally:
        gpu.lib().rodent_hip_top_min_rays(-1)


def variants(gpu, width):
    v = gpu.order_preserving_variants(width)
    assert [gpu.variants(width)[i] for i in v] == ["top", "single", "single-noxcd"]
    return v


def assert_same(got, ref, what):
    a, b = got.view("<u4").reshape(-1, 4), ref.view("<u4").reshape(-1, 4)
    assert a.shape == b.shape, what
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ref)} records differ, first ray {bad[0]}: {got[bad[0]]} vs {ref[bad[0]]}"


def handed_off(gpu, bvh, rays, any_hit, variant):
    """(hits, rays that k_wide_finish took from the deep list) of one launch: stats word 7 (k_wide_finish adds deep_count)."""
    gpu.traverse(bvh, rays[:1], any_hit=any_hit, variant=variant)      # read_stats reads the context of the latest launch: this stream's
    gpu.read_stats()
    got = gpu.traverse(bvh, rays, any_hit=any_hit, variant=variant)
    return got, int(gpu.read_stats()[7])


# (name, any hit, chain_last, miss_every, ties): the last two only where the fan allows (ties need two leaves per level)
TREES = (("closest", False, False, False, False),
         ("closest-ties", False, True, True, True),
         ("any", True, True, True, False))


def build_tree(width, peak, fan, chain_last, miss, ties):
    """chain_wide with a stack peak of exactly `peak` entries -> (nodes, tris, whether it has ties)."""
    ties = ties and fan >= 2
    depth = -(-peak // fan)
    last = peak - (depth - 1) * fan
    k = W.miss_every_for(depth, fan, last, ties) if miss else 0
    nodes, tris = W.chain_wide(width, depth, fan, chain_last=chain_last, miss_every=k, ties=ties, last_fan=last)
    assert W.chain_counts(depth, fan, last, ties)[2] == peak
    return nodes, tris, ties


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fan", [1, "arity-1"])
@pytest.mark.parametrize("peak", ["window-1", "window", "window+1", 40, 62, 63])
def test_depths_around_the_window_and_up_to_capacity(gpu, oracle, width, fan, peak):
    """Stack peaks of LDS_N - 1 (the last one that stays in the window), LDS_N, LDS_N + 1, 40, 62 and 63 (the reference's capacity)
    entries; one leaf per level and arity - 1 (one node step jumps several rows across the window's end into the spare rows);
    closest hit, closest hit with duplicated triangles in equal sibling boxes and rejecting packets, any hit with occluders moved
    away; 30 000 rays of which a third miss, coherent and shuffled; every launch twice (the second runs on the control words and
    ticket counters that the first one's k_wide_finish reset)."""
    window = W.LDS_WINDOW[width]
    fan = width - 1 if fan == "arity-1" else fan
    peak = {"window-1": window - 1, "window": window, "window+1": window + 1}.get(peak, peak)
    n = 30000
    ray_sets = {"coherent": W.chain_rays(n, peak), "shuffled": W.chain_rays(n, peak + 100, jitter=True, shuffle=True)}
    for name, any_hit, chain_last, miss, ties in TREES:
        nodes, tris, ties = build_tree(width, peak, fan, chain_last, miss, ties)
        bvh = gpu.DeviceBvh(width, nodes, tris, 0)
        for set_name, rays in ray_sets.items():
            ref, st = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
            assert st["max_stack"] == peak + 1 and (ref["tri_id"] >= 0).sum() > n // 2
            if ties:
                assert set(ref["tri_id"][ref["tri_id"] >= 0]) <= {0, 1}        # the duplicated pair of level 0
            for min_rays in FORMS:
                with form(gpu, min_rays):
                    for v in variants(gpu, width):
                        for rep in range(2):
                            got = gpu.traverse(bvh, rays, any_hit=any_hit, variant=v)
                            assert_same(got, ref, f"BVH{width} peak {peak} fan {fan} {name} {set_name} top_min_rays({min_rays}) "
                                                  f"{gpu.variants(width)[v]} launch {rep}")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fan", [1, "arity-1"])
def test_the_hand_off_is_counted_exactly(gpu, oracle, width, fan):
    """wide_chunk abandons a ray iff a node step leaves the top of its stack at row >= LDS_N, i.e. iff the ray's own stack peak
    (max_stack of a one-ray oracle call minus the sentinel) reaches LDS_N; k_wide_finish adds the length of the deep list to stats
    word 7.  So a launch hands off exactly the rays whose peak is >= LDS_N: none on a tree of peak LDS_N - 1, every ray that enters
    the chain at LDS_N.  Half of the entering rays here have a tmax inside the chain, which keeps the leaves behind it off their
    stack: their peaks are spread around the window's end."""
    window = W.LDS_WINDOW[width]
    fan = width - 1 if fan == "arity-1" else fan
    n = 4096
    for peak in (window - 1, window, window + 1, 40):
        rays = W.chain_rays(n, 7 * peak + fan, jitter=True, cut=(W.Z0 - 5, W.Z0 + peak + 5))
        enters_uncut = (np.abs(rays["org"][:, 0]) < 5) & (rays["tmax"] == np.float32(1000.0))
        for name, any_hit, chain_last, miss, ties in TREES:
            nodes, tris, ties = build_tree(width, peak, fan, chain_last, miss, ties)
            bvh = gpu.DeviceBvh(width, nodes, tris, 0)
            ref, _ = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
            peaks = W.ray_peaks(oracle, width, nodes, tris, rays, any_hit)
            expected = int((peaks >= window).sum())
            # what the derivation says about this fixture, before the GPU is asked
            assert peaks.max() == peak and (peaks[enters_uncut] == peak).all() and enters_uncut.sum() > n // 4
            if peak < window:
                assert expected == 0
            else:
                assert enters_uncut.sum() <= expected < (np.abs(rays["org"][:, 0]) < 5).sum()
            for min_rays in FORMS:
                with form(gpu, min_rays):
                    for v in variants(gpu, width):
                        got, count = handed_off(gpu, bvh, rays, any_hit, v)
                        what = f"BVH{width} peak {peak} fan {fan} {name} top_min_rays({min_rays}) {gpu.variants(width)[v]}"
                        print(f"{what}: {count} rays handed off, {expected} rays with a peak >= {window}")
                        assert_same(got, ref, what)
                        assert count == expected, what


@pytest.mark.parametrize("width", WIDTHS)
def test_stack_overflow_is_reported_not_silent(gpu, oracle, width):
    """64 entries do not fit the reference's 64 slots (one is the sentinel).  The rays reach k_wide_finish like any deep ray; there
    DeepStack::put drops a push to row >= 64 and raises the flag, DeepStack::get clamps its row to 63 -- no access outside the 64
    rows -- and the rows only ever hold leaves of this tree, so the ray still ends.  Through the asynchronous entry + check_errors:
    reported once, cleared, and a 63-entry launch right after it is exact.  (The synchronous reference-named entry points abort()
    on the flag: not used here.)"""
    rays = W.chain_rays(200, 2, miss_third=False)
    for any_hit in (False, True):
        for fan in (1, width - 1):
            (nodes, tris), _ = W.chain_wide_peak(width, 64, fan, chain_last=any_hit)
            with pytest.raises(RuntimeError, match="stack overflow"):
                oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
            (ok_nodes, ok_tris), _ = W.chain_wide_peak(width, 63, fan, chain_last=any_hit)
            ref, st = oracle.traverse(width, ok_nodes, ok_tris, rays, any_hit=any_hit, algo="gpu")
            assert st["max_stack"] == 64
            over, ok = gpu.DeviceBvh(width, nodes, tris, 0), gpu.DeviceBvh(width, ok_nodes, ok_tris, 0)
            for min_rays in FORMS:
                with form(gpu, min_rays):
                    for v in variants(gpu, width):
                        assert v is not None
                        with pytest.raises(RuntimeError, match="stack overflow"):
                            gpu.traverse(over, rays, any_hit=any_hit, variant=v)
                        assert gpu.lib().rodent_hip_check_errors(0, None) == 0          # cleared by the report
                        got, count = handed_off(gpu, ok, rays, any_hit, v)
                        assert_same(got, ref, f"BVH{width} 63 entries after an overflow, fan {fan} any={any_hit} "
                                              f"top_min_rays({min_rays}) {gpu.variants(width)[v]}")
                        assert count == len(rays)


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345,
                     0x40A00000, 0xBF800000, 0x3C23D70A, 0x7F7FFFFF], dtype="<u4").view("<f4")


def with_special_ranges(rays):
    """Four rays for each of the 144 (tmin, tmax) pairs of test_gpu_parity.test_special_tmin_tmax_values."""
    rays = rays[:len(SPECIALS) ** 2 * 4].copy()
    assert len(rays) == 576
    k = np.arange(len(rays))
    rays["tmin"] = SPECIALS[k % len(SPECIALS)]
    rays["tmax"] = SPECIALS[(k // len(SPECIALS)) % len(SPECIALS)]
    return rays


@pytest.mark.parametrize("width", WIDTHS)
def test_special_tmin_tmax_values(gpu, oracle, cornell, width):
    """tmin / tmax from {0, -0, denormal, +-inf, quiet NaN, signalling NaN, ...}: fminf / fmaxf ignore a NaN bound, the triangle
    test's comparisons reject it.  wide_chunk issues raw v_max_f32 / v_min_f32 on canonicalised bounds, writes the miss record from
    the uncanonicalised tmax and splits the triangle test at t <= abs_det * tmax; wide_ray_literal does none of that.  Both must
    give the oracle's bytes, the NaN payload of a miss record included: on the Cornell box (in-window) and on a 40-entry chain
    (follow-up kernel).  Any hit too: the wide loops keep the reference's visit order, so the occluder found is the oracle's."""
    cases = {"cornell": cornell.blocks[width] + (with_special_ranges(cornell.ray_sets["primary"]),)}
    chain = W.chain_rays(576, 5, miss_third=False, jitter=True)
    chain["org"][432:, 0] += 50.0                                  # the fourth ray of every pair misses the chain
    for name, any_hit, chain_last, miss, ties in TREES:
        nodes, tris, _ = build_tree(width, 40, width - 1, chain_last, miss, ties)
        cases[f"chain-{name}"] = (nodes, tris, with_special_ranges(chain))
    for case, (nodes, tris, rays) in cases.items():
        bvh = gpu.DeviceBvh(width, nodes, tris, 0)
        for any_hit in (False, True):
            ref, st = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
            deep = W.ray_peaks(oracle, width, nodes, tris, rays, any_hit) >= W.LDS_WINDOW[width]
            if case == "cornell":
                assert not deep.any()
            elif any_hit and case != "chain-closest":              # (chain in slot 0: an occlusion ray stays shallow)
                # a leaf is pushed iff tmin <= z <= tmax, NaN bounds ignored: 10 values of tmin x 5 of tmax (inf, FLT_MAX, three
                # NaNs) x 3 rays in the chain; the triangle test rejects a NaN bound: the miss record carries the NaN
                assert deep.sum() == 150 and (ref["tri_id"][deep] < 0).sum() == 108 and np.isnan(ref["t"][deep]).sum() == 90
            elif not any_hit:
                # closest hit: `tentry < tnear` starts from tnear = tmax, so with a NaN tmax no child ever becomes the top and the
                # ray ends at the root (the reference's loop, literally): deep are 10 x 2 (inf, FLT_MAX) x 3, the NaN tmin miss
                assert deep.sum() == 60 and (ref["tri_id"][deep] < 0).sum() == 18
            for min_rays in FORMS:
                with form(gpu, min_rays):
                    for v in variants(gpu, width):
                        got, count = handed_off(gpu, bvh, rays, any_hit, v)
                        what = f"BVH{width} {case} any={any_hit} top_min_rays({min_rays}) {gpu.variants(width)[v]}"
                        assert_same(got, ref, what)
                        assert count == deep.sum(), what


@pytest.mark.parametrize("width", WIDTHS)
def test_launches_on_several_streams_may_overlap(gpu, oracle, width):
    """Every (device, stream) owns its deep list and deep_count: four streams trace different ray sets and counts on one 40-entry
    chain at the same time, same and mixed mappings in flight, closest and any hit in turn, five times over; all exact, no error
    flag on any stream."""
    import torch
    nodes, tris, ties = build_tree(width, 40, width - 1, True, True, True)
    assert ties
    bvh = gpu.DeviceBvh(width, nodes, tris, 0)
    sets = []
    for k in range(4):
        n = 20000 + 777 * k
        rays = W.chain_rays(n, 11 + k, jitter=True)
        refs = [oracle.traverse(width, nodes, tris, rays, any_hit=a, algo="gpu")[0] for a in (False, True)]
        sets.append((rays, refs, gpu.to_device(rays, 0), torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0"), torch.cuda.Stream()))
    torch.cuda.synchronize()
    vs = variants(gpu, width)
    for min_rays in FORMS:
        with form(gpu, min_rays):
            for rep in range(5):
                any_hit = bool(rep % 2)
                for v in vs:
                    for rays, refs, rd, hd, st in sets:
                        hd.fill_(0xFF)
                    torch.cuda.synchronize()
                    for k, (rays, refs, rd, hd, st) in enumerate(sets):
                        gpu.traverse_async(bvh, rd, hd, len(rays), any_hit, vs[(v + k) % len(vs)] if rep >= 2 else v, st)
                    torch.cuda.synchronize()
                    for k, (rays, refs, rd, hd, st) in enumerate(sets):
                        assert_same(gpu.from_device(hd, F.HIT1), refs[any_hit], f"BVH{width} stream {k} rep {rep} any={any_hit} "
                                                                                f"top_min_rays({min_rays}) {gpu.variants(width)[v]}")
                for st in (s[4] for s in sets):
                    assert gpu.lib().rodent_hip_check_errors(0, ctypes.c_void_p(st.cuda_stream)) == 0


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ragged_launches_where_every_ray_is_deep(gpu, oracle, width, n):
    """Every ray of the launch is handed off: the deep list is as long as the launch (it is sized n)."""
    nodes, tris, _ = build_tree(width, 40, width - 1, True, True, True)
    bvh = gpu.DeviceBvh(width, nodes, tris, 0)
    rays = W.chain_rays(n, n, miss_third=False, jitter=True)
    for any_hit in (False, True):
        ref, _ = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
        assert (ref["tri_id"] >= 0).all()
        for min_rays in FORMS:
            with form(gpu, min_rays):
                for v in variants(gpu, width):
                    got, count = handed_off(gpu, bvh, rays, any_hit, v)
                    what = f"BVH{width} n {n} any={any_hit} top_min_rays({min_rays}) {gpu.variants(width)[v]}"
                    assert_same(got, ref, what)
                    assert count == n, what


@pytest.mark.parametrize("width", WIDTHS)
def test_a_large_launch_where_every_ray_is_deep(gpu, oracle, width):
    """600 000 deep rays through the persistent form: every one of k_wide_finish's workgroups takes several batches of the deep
    list, every wave of k_wide_top_persist several tickets."""
    n = 600_000
    nodes, tris, _ = build_tree(width, 40, width - 1, True, True, True)
    bvh = gpu.DeviceBvh(width, nodes, tris, 0)
    rays = W.chain_rays(n, 600, miss_third=False, jitter=True)
    ref, _ = oracle.traverse(width, nodes, tris, rays, algo="gpu")
    assert (ref["tri_id"] >= 0).all()
    top = gpu.variants(width).index("top")
    assert gpu.kernel_name(width, top).startswith("k_wide_top_persist")
    with form(gpu, 0):
        for rep in range(2):
            got, count = handed_off(gpu, bvh, rays, False, top)
            assert_same(got, ref, f"BVH{width} 600 000 deep rays, launch {rep}")
            assert count == n


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ["primary", "random"])
def test_how_deep_the_atrium_goes(gpu, oracle, width, kind):
    """A measurement, not a bar: the deepest stack of the two benchmark ray sets in the atrium's wide blocks (64 Ki-ray sample,
    every 16th ray) and how many of those rays a launch hands to k_wide_finish -- which must be the rays whose own peak reaches the
    window, as in test_the_hand_off_is_counted_exactly.  The figures are recorded in LAB_NOTES.md."""
    from rodent_amd import scenes, raygen
    path = scenes.scene_bvh("atrium")
    nodes, tris = F.read_bvh(path, {4: F.BVH4_TRI4, 8: F.BVH8_TRI4}[width])
    if kind == "primary":
        eye, d, up, fov = scenes.CAMERAS["atrium"]
        rays = raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, 5000.0)[::16]
    else:
        lo, hi = raygen.scene_bounds(F.read_bvh(path, F.BVH4_TRI4)[0])
        rays = raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, 1.0)[::16]
    assert len(rays) == 65536
    window = W.LDS_WINDOW[width]
    bvh = gpu.DeviceBvh(width, nodes, tris, 0)
    for any_hit in (False, True):
        ref, st = oracle.traverse(width, nodes, tris, rays, any_hit=any_hit, algo="gpu")
        deepest = st["max_stack"] - 1
        # one-ray oracle calls only where some ray can have reached the window
        expected = int((W.ray_peaks(oracle, width, nodes, tris, rays, any_hit) >= window).sum()) if deepest >= window else 0
        for min_rays in FORMS:
            with form(gpu, min_rays):
                got, count = handed_off(gpu, bvh, rays, any_hit, gpu.variants(width).index("top"))
            print(f"atrium BVH{width} {kind} {'any' if any_hit else 'closest'} top_min_rays({min_rays}): deepest stack {deepest} "
                  f"entries (window {window}), {count} of {len(rays)} rays handed to k_wide_finish, {expected} expected")
            assert_same(got, ref, f"atrium BVH{width} {kind} any={any_hit} top_min_rays({min_rays})")
            assert count == expected
