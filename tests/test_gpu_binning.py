"""The renderer's binning stage (render_sort.h: k_bin_count, k_bin_scan_blocks, k_bin_scan_bins, k_scatter) through hip_bin_primary,
slab for slab against the stable sort of tests/binning_model.py.

Nothing here takes a tolerance: the stage permutes 32-bit words.  Every word of `from` is unique per (array, ray) -- but for the key
array -- so an exchange of two arrays or of two rays shows; `to` and the index array start as 0xCDCDCDCD.  After every call the whole
`to` slab up to its capacity, `from` (unchanged), the index array with its tail, the bin ends and the returned count are compared.
Keys stay inside [0, num_bins) and the device-side size never exceeds max_n (the entry's precondition)."""
import ctypes as C
import time

import numpy as np
import pytest

import binning_model as BM
import shade_fixtures as SF

pytestmark = pytest.mark.gpu
BLOCK = BM.BLOCK                                                 # rays per binning block
CAP = 3 * BLOCK + 64                                             # streams of the small cases
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1024 + 256, 1024 + 257, 1024 + 769, 2049)
SENTINEL_I32 = int(np.array([SF.SENTINEL]).view("<i4")[0])
# (mode, num_bins, drop_from_bin, keep_hit, copy_interval, index-only) with G = 9 geometries
LOOP_SORT, LOOP_SORT_INDEX, STAGE_SORT = (0, 10, 9, 1, 0, False), (0, 10, 9, 1, 0, True), (0, 10, 10, 1, 1, False)
LOOP_COMPACTION = (1, 2, 1, 0, 1, False)
FORMS = {"loop sort": LOOP_SORT, "loop sort, index only": LOOP_SORT_INDEX, "stage sort": STAGE_SORT, "loop compaction": LOOP_COMPACTION}


@pytest.fixture(scope="module")
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


def streams(R, cap_p, cap_q):
    l = R.stage_lib()
    p, q = R.PrimaryStream(), R.PrimaryStream()
    l.rodent_gpu_get_first_primary_stream(0, C.byref(p), cap_p)
    l.rodent_gpu_get_second_primary_stream(0, C.byref(q), cap_q)
    assert SF.slab_cap(p) >= cap_p and SF.slab_cap(q) >= cap_q
    return l, p, q


@pytest.fixture()
def small(R):
    return streams(R, CAP, CAP)


def unique_words(rows, cap):
    return (np.asarray(rows, "<u4")[:, None] << 26 | np.arange(cap, dtype="<u4")[None, :]).astype("<u4")


def with_keys(slab, keys, mode):
    """The key array of a `from` slab: geom_id = key, or id >= 0 (key 0) / id < 0 (key 1), ids distinct either way."""
    i = np.arange(len(keys), dtype="<i4")
    if mode == 0:
        slab[SF.GEOM, :len(keys)] = np.asarray(keys, "<i4").view("<u4")
    else:
        slab[SF.ID, :len(keys)] = np.where(np.asarray(keys) == 0, i, ~i).astype("<i4").view("<u4")
    return slab


def narrowed(keys, n, num_bins, drop, perm):
    """Which of the three terms of a slot the first misplaced ray of an index-only result is off by (binning_model.slot_decomposition)."""
    keys = np.asarray(keys)[:n]
    begin, earlier, rank = BM.slot_decomposition(keys, n, num_bins)
    slot = np.full(n, -1, np.int64)
    at = np.flatnonzero((perm >= 0) & (perm < n))
    slot[perm[at]] = at
    kept = np.flatnonzero(keys < drop)
    bad = kept[slot[kept] != (begin + earlier + rank)[kept]]
    if not len(bad):
        return "every kept ray is at its slot; the index array differs elsewhere"
    i = int(bad[0])
    return f"{len(bad)} rays off their slot, first ray {i} (key {keys[i]}, block {i // BLOCK}): slot {slot[i]}, model: bin begin " \
           f"{begin[i]} + earlier blocks {earlier[i]} + rank {rank[i]}"


def run(R, l, p, q, what, keys, n, form, max_n=None, device_size=False, stream=None):
    """One call of hip_bin_primary on fresh slabs, everything it leaves behind against the model.  `keys`: max_n keys (the rays behind n
    carry keys too).  Returns the `to` slab."""
    import torch
    mode, num_bins, drop, keep_hit, copy_interval, index_only = form
    max_n = n if max_n is None else max_n
    assert len(keys) == max_n >= n and SF.slab_cap(p) >= max_n and SF.slab_cap(q) >= max_n
    f0 = with_keys(unique_words(range(SF.P_ROWS), SF.slab_cap(p)), keys, mode)
    t0 = SF.sentinel(q, SF.P_ROWS)
    SF.write_slab(R, p, f0); SF.write_slab(R, q, t0)
    perm0 = np.full(max_n + 64, SENTINEL_I32, "<i4")
    d_perm = torch.from_numpy(perm0).cuda() if index_only else None
    d_size = torch.tensor([n], dtype=torch.int32, device="cuda") if device_size else None
    torch.cuda.synchronize()
    ends = (C.c_int32 * num_bins)()
    got = l.hip_bin_primary(0, C.byref(p), C.byref(q), mode, num_bins, drop, keep_hit, copy_interval,
        d_perm.data_ptr() if index_only else None, d_size.data_ptr() if device_size else None, max_n, ends, stream)
    f1, t1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, q, SF.P_ROWS)
    want_t, want_perm, want_ends = BM.binned(f0, t0, keys, n, num_bins, drop, keep_hit, copy_interval, perm0 if index_only else None)
    assert list(ends) == want_ends.tolist(), f"{what}: bin ends"
    assert got == want_ends[drop - 1], f"{what}: returned count"
    if index_only:
        perm1 = d_perm.cpu().numpy()
        assert np.array_equal(perm1, want_perm), f"{what}: index array: {narrowed(keys, n, num_bins, drop, perm1)}"
    SF.assert_same(t1, want_t, what + ", `to`")
    SF.assert_same(f1, f0, what + ", `from`")
    return t1


def keys_of(form, n, rng):
    return rng.integers(0, form[1], n)


# ---- a. every word moves with its ray, and nothing else moves ----------------------------------------------
@pytest.mark.parametrize("name", list(FORMS))
def test_every_word_moves_with_its_ray(R, small, name):
    """Stream sizes around the wave, the 256 threads of a counting workgroup (four rays each, 256 apart) and the 1024-ray block, in
    the forms the renderer's loop and the stage entries launch."""
    rng = np.random.default_rng(len(name))
    for n in SIZES:
        run(R, *small, f"{name}, {n} rays", keys_of(FORMS[name], n, rng), n, FORMS[name])


@pytest.mark.parametrize("mode,keep_hit,copy_interval", [(0, 0, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (1, 0, 0)])
def test_remaining_copy_switches(R, small, mode, keep_hit, copy_interval):
    """The keep_hit / copy_interval combinations no launch of the library uses, once each."""
    rng = np.random.default_rng(7)
    form = (mode, 10 if mode == 0 else 2, 9 if mode == 0 else 1, keep_hit, copy_interval, False)
    n = BLOCK + 257
    run(R, *small, f"mode {mode}, keep_hit {keep_hit}, copy_interval {copy_interval}, {n} rays", keys_of(form, n, rng), n, form)


# ---- b. keys that drive the ballot rounds to their edges ------------------------------------------------------
@pytest.mark.parametrize("num_bins", [2, 3, 10, 64, 65, 1024, 1025])
def test_key_patterns(R, small, num_bins):
    """Two full blocks and a partial one (300 rays) under every pattern of binning_model.key_patterns: up to 64 ballot rounds in a wave,
    keys that change at lane 0 and at lane 32, a key that only the partial block holds, empty bins, everything dropped; copying with the
    last bin dropped (the loop's sort) and index-only with nothing dropped."""
    rng = np.random.default_rng(num_bins)
    n = 2 * BLOCK + 300
    for pattern, keys in BM.key_patterns(n, num_bins, rng).items():
        run(R, *small, f"{num_bins} bins, {pattern}, last bin dropped", keys, n, (0, num_bins, num_bins - 1, 1, 0, False))
        run(R, *small, f"{num_bins} bins, {pattern}, index only", keys, n, (0, num_bins, num_bins, 1, 1, True))


# ---- c. device-side size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_n", [2 * BLOCK, 3 * BLOCK])
def test_size_behind_a_device_pointer(R, small, max_n):
    """The stream size read from device memory, launches sized by max_n: the rays behind the size carry keys (alive and dead ids) that
    would change every count and slot if a kernel read them."""
    rng = np.random.default_rng(max_n)
    for n in (max_n, max_n - 1, BLOCK, BLOCK + 1, 0):
        for name in ("loop compaction", "loop sort", "loop sort, index only"):
            run(R, *small, f"{name}, size {n} on the device, max_n {max_n}", keys_of(FORMS[name], max_n, rng), n, FORMS[name],
                max_n=max_n, device_size=True)


# ---- e. twice the same bytes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loop sort", "stage sort", "loop compaction"])
def test_twice_the_same_bytes(R, small, name):
    """The same rays binned from the second slab into the first, on another HIP stream and with the per-block counts of the run before
    still in the scratch array: the same slab."""
    import torch
    l, p, q = small
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream()
    for n in (BLOCK + 769, 2049):
        keys = keys_of(FORMS[name], n, rng)
        first = run(R, l, p, q, f"{name}, {n} rays", keys, n, FORMS[name])
        again = run(R, l, q, p, f"{name}, {n} rays, second run", keys, n, FORMS[name], stream=side.cuda_stream)
        SF.assert_same(again, first, f"{name}, {n} rays, second run against the first")
    torch.cuda.synchronize()


# ---- d. the scan over per-block counts ----------------------------------------------------------------------------
BIG_BLOCKS = (15, 16, 17, 31, 33, 4095, 4096, 4097, 4128, 8200)
COPY_BLOCKS = 4097
SECONDS = 5.0                                                    # what one large case may take, model and copies included


@pytest.fixture(scope="module")
def big(R):
    """The two slabs of the large cases, allocated once: 8200 blocks for the index-only runs (which bin a stream onto itself), 4097
    for the one copying run."""
    return streams(R, max(BIG_BLOCKS) * BLOCK, COPY_BLOCKS * BLOCK)


@pytest.mark.parametrize("num_blocks", BIG_BLOCKS)
def test_scan_over_block_counts(R, big, num_blocks):
    """k_bin_scan_blocks: three bins, index-only, 1024 * num_blocks - 5 rays.  16 counts per thread as four 16-byte loads where a thread's
    run is whole and the bin's row aligned, one by one otherwise (odd block counts: the rows of bins 1 and 2 are unaligned; 17 and 33: both
    paths in one tile), a carry across tiles of 4096 counts (4097, 4128 -- vector path in the second tile -- and 8200: three tiles)."""
    import torch
    started = time.perf_counter()
    l, p, _ = big
    n = BLOCK * num_blocks - 5
    keys = np.random.default_rng(num_blocks).integers(0, 3, n).astype("<i4")
    R.write_stream_array(p.geom_id, keys)
    d_perm = torch.full((n + 64,), SENTINEL_I32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ends = (C.c_int32 * 3)()
    got = l.hip_bin_primary(0, C.byref(p), C.byref(p), 0, 3, 2, 1, 0, d_perm.data_ptr(), None, n, ends, None)
    perm1 = d_perm.cpu().numpy()
    _, want_perm, want_ends = BM.binned(None, None, keys, n, 3, 2, 1, 0, np.full(n + 64, SENTINEL_I32, "<i4"))
    what = f"{num_blocks} blocks"
    assert list(ends) == want_ends.tolist(), what
    assert got == want_ends[1], what
    assert np.array_equal(perm1, want_perm), f"{what}: {narrowed(keys, n, 3, 2, perm1)}"
    assert np.array_equal(R.read_stream_array(p.geom_id, n, "<i4"), keys), what + ": the keys changed"
    seconds = time.perf_counter() - started
    print(f"{what}: {seconds:.2f} s")
    assert seconds < SECONDS, what


def test_copy_across_two_scan_tiles(R, big):
    """The loop's copying sort at 4097 blocks (the carry of the scan in every slot of the second tile's block): id, rnd and depth of
    `to` against the model, with the untouched entries behind the rays kept."""
    started = time.perf_counter()
    l, p, q = big
    n = BLOCK * COPY_BLOCKS - 5
    m = n + 32                                                   # with entries behind the stream, inside `to`'s capacity
    assert m <= SF.slab_cap(q)
    rows = {"id": (p.rays.id, q.rays.id, SF.ID), "rnd": (p.rnd, q.rnd, SF.RND), "depth": (p.depth, q.depth, SF.DEPTH)}
    keys = np.random.default_rng(5).integers(0, 3, n).astype("<i4")
    src = unique_words([row for _, _, row in rows.values()], m)
    R.write_stream_array(p.geom_id, keys)
    for k, (from_ptr, to_ptr, _) in enumerate(rows.values()):
        R.write_stream_array(from_ptr, src[k])
        R.write_stream_array(to_ptr, np.full(m, SF.SENTINEL, "<u4"))
    ends = (C.c_int32 * 3)()
    got = l.hip_bin_primary(0, C.byref(p), C.byref(q), 0, 3, 2, 1, 0, None, None, n, ends, None)
    # (the three rows move whatever the switches say: the model is asked for a plain copy of a three-row slab)
    want, _, want_ends = BM.binned(src, np.full_like(src, SF.SENTINEL), keys, n, 3, 2, 1, 1)
    assert list(ends) == want_ends.tolist() and got == want_ends[1]
    for k, (name, (from_ptr, to_ptr, _)) in enumerate(rows.items()):
        SF.assert_same(R.read_stream_array(to_ptr, m, "<u4")[None], want[k][None], f"{name} of `to`")
        SF.assert_same(R.read_stream_array(from_ptr, m, "<u4")[None], src[k][None], f"{name} of `from`")
    seconds = time.perf_counter() - started
    print(f"copying sort at {COPY_BLOCKS} blocks: {seconds:.2f} s")
    assert seconds < SECONDS
