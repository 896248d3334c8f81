"""CPU model of the renderer's binning stage (rodent_amd/csrc/render_sort.h: k_bin_count, k_bin_scan_blocks, k_bin_scan_bins, k_scatter,
launched by bin_stream; include/rodent_render.h: hip_bin_primary) in numpy.

The stage is a stable counting sort of a primary stream by a small integer key, so its whole specification is `np.argsort(kind="stable")`
plus the list of arrays that move: `binned` says what a call leaves in `to`, in `perm` and in the bin ends, as 32-bit words.
`slot_decomposition` restates the three terms the kernels add up to a ray's slot, so that a failing case can be narrowed to one launch;
`key_patterns` are the key sequences that put the in-wave ballot rounds, the in-block ranking and the per-block counts on their edges.
A slab is a uint32 array (rows, cap) in carve order, as in shade_fixtures."""
from __future__ import annotations

import numpy as np

TMIN, TMAX = 7, 8
HIT_ROWS = slice(9, 14)
BLOCK, WAVE = 1024, 64                                           # kBinBlock, kWave


def stable_order(keys):
    """Stream indices in slot order: by key, ties in stream order."""
    keys = np.asarray(keys)
    # (a 16-bit key takes numpy's radix sort: the 8 Mi-ray cases stay cheap)
    return np.argsort(keys.astype(np.int16) if len(keys) and keys.max() < 2 ** 15 else keys, kind="stable")


def binned(from_slab, to_before, keys, n, num_bins, drop_from_bin, keep_hit, copy_interval, perm_before=None):
    """What binning the first n rays of `from_slab` by `keys` leaves behind: (to_after, perm_after, ends).
    With `perm_before` (index-only sort) `to` is returned as it was -- the slabs may then be None -- and perm_after[d] is the stream
    index of the ray in slot d; without, perm_after is None and every row of `to` takes from[row, order], except the five hit rows when
    keep_hit == 0 and tmin / tmax when copy_interval == 0.  Those rows, and everything behind the rays kept, keep `to_before`."""
    keys = np.asarray(keys)[:n].astype(np.int64)
    assert 1 <= drop_from_bin <= num_bins and (len(keys) == 0 or (0 <= keys.min() and keys.max() < num_bins))
    order = stable_order(keys)
    order = order[:int((keys < drop_from_bin).sum())]             # sorted by key: the kept rays are a prefix
    ends = np.cumsum(np.bincount(keys, minlength=num_bins)).astype(np.int64)
    if perm_before is not None:
        perm_after = perm_before.copy()
        perm_after[:len(order)] = order.astype(perm_before.dtype)
        return to_before, perm_after, ends
    to_after = to_before.copy()
    moved = np.ones(to_before.shape[0], bool)
    if not keep_hit:
        moved[HIT_ROWS] = False
    if not copy_interval:
        moved[[TMIN, TMAX]] = False
    rows = np.flatnonzero(moved)
    to_after[rows[:, None], np.arange(len(order))[None, :]] = from_slab[rows[:, None], order[None, :]]
    return to_after, None, ends


def slot_decomposition(keys, n, num_bins, block=BLOCK):
    """Per ray the three terms of its slot, as the kernels compute them: (bin begin -- k_bin_scan_bins; rays of that key in earlier
    blocks -- k_bin_count + k_bin_scan_blocks; rank among the block's rays of that key -- block_rank in k_scatter)."""
    keys = np.asarray(keys)[:n].astype(np.int64)
    blk = np.arange(n) // block
    num_blocks = max(1, -(-n // block))
    hist = np.zeros((num_bins, num_blocks), np.int64)             # [bin][block], the layout of the device array
    np.add.at(hist, (keys, blk), 1)
    totals = hist.sum(1)
    bin_begin = np.cumsum(totals) - totals
    earlier = np.cumsum(hist, 1) - hist
    comb = blk * num_bins + keys
    order = np.argsort(comb, kind="stable")
    first = np.searchsorted(comb[order], comb[order], "left")     # where the run of this (block, key) starts
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - first
    return bin_begin[keys], earlier[keys, blk], rank


def key_patterns(n, num_bins, rng, block=BLOCK, wave=WAVE):
    """name -> n keys in [0, num_bins)."""
    i = np.arange(n)
    last, mid = num_bins - 1, (num_bins // 2 if num_bins > 2 else 1)
    out = {"all rays the first key": np.zeros(n, np.int64), "all rays the last key": np.full(n, last, np.int64),
           # 64 distinct keys in a wave from 64 bins on: one ballot round per lane
           "i mod bins": i % num_bins,
           # one round per wave; the key changes between lane 63 and lane 0
           "one key per wave": (i // wave) % num_bins,
           # ... and between lanes 31 and 32
           "one key per half wave": (i // (wave // 2)) % num_bins,
           "descending": last - i % num_bins}
    # a key that only the final (partial) block holds: its count is zero in every earlier block
    k = np.zeros(n, np.int64)
    tail = i >= (max(n, 1) - 1) // block * block
    k[tail & (i % 3 == 1)] = mid
    out["a key only in the final block"] = k
    # empty bins in the middle (from three bins on): the first and the last key only
    out["first and last key only"] = np.where(rng.random(n) < 0.4, 0, last)
    # the last key (which the loop's sort drops; "all rays the last key" is then the empty result) but for two lanes per wave
    out["the last key, twice per wave the first"] = np.where(i % (wave // 2) == 5, 0, last)
    out["skewed random"] = np.minimum(last, np.floor(num_bins * rng.random(n) ** 4)).astype(np.int64)
    out["uniform random"] = rng.integers(0, num_bins, n)
    return out
