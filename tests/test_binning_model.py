"""The numpy model of the binning stage (tests/binning_model.py) against answers written out by hand, and its slot decomposition --
bin begin + rays of the key in earlier blocks + rank in the block, the three terms the kernels add -- against the stable argsort on the
key patterns tests/test_gpu_binning.py runs on the device, at a reduced block and wave size."""
import numpy as np
import pytest

import binning_model as BM

ROWS = 20


def slab(cap, base=0):
    """Every word unique per (row, entry)."""
    return (np.arange(ROWS, dtype="<u4")[:, None] << 26 | (base + np.arange(cap, dtype="<u4"))[None, :]).astype("<u4")


#          ray   0  1  2  3  4  5  6  7  8  9 10 11
KEYS = np.array([2, 0, 3, 1, 0, 2, 2, 3, 0, 1, 2, 0])
ORDER = [1, 4, 8, 11, 3, 9, 0, 5, 6, 10, 2, 7]                   # key 0: rays 1 4 8 11; key 1: 3 9; key 2: 0 5 6 10; key 3: 2 7
ENDS = [4, 6, 10, 12]


def test_a_dozen_rays_by_hand():
    f, t0 = slab(16), np.full((ROWS, 16), 0xCDCDCDCD, "<u4")
    t, perm, ends = BM.binned(f, t0, KEYS, 12, 4, 4, 1, 1)
    assert perm is None and ends.tolist() == ENDS
    assert np.array_equal(t[:, :12], f[:, ORDER]) and np.array_equal(t[:, 12:], t0[:, 12:])
    # the loop's sort: bin 3 (the rays that missed) dropped, the ray interval left behind
    t, _, ends = BM.binned(f, t0, KEYS, 12, 4, 3, 1, 0)
    assert ends.tolist() == ENDS
    for row in range(ROWS):
        want = t0[row] if row in (7, 8) else np.concatenate([f[row, ORDER[:10]], t0[row, 10:]])
        assert np.array_equal(t[row], want), row
    # keep_hit == 0: rows 9 ... 13 stay
    t, _, _ = BM.binned(f, t0, KEYS, 12, 4, 4, 0, 1)
    for row in range(ROWS):
        want = t0[row] if 9 <= row <= 13 else np.concatenate([f[row, ORDER], t0[row, 12:]])
        assert np.array_equal(t[row], want), row
    # only the first seven rays: 2 0 3 1 0 2 2
    t, _, ends = BM.binned(f, t0, KEYS, 7, 4, 3, 1, 1)
    assert ends.tolist() == [2, 3, 6, 7]
    assert np.array_equal(t[:, :6], f[:, [1, 4, 3, 0, 5, 6]]) and np.array_equal(t[:, 6:], t0[:, 6:])


def test_index_only_by_hand():
    p0 = np.full(16, -842150451, "<i4")
    t, perm, ends = BM.binned(None, None, KEYS, 12, 4, 3, 1, 0, p0)
    assert t is None and ends.tolist() == ENDS
    assert perm.tolist() == ORDER[:10] + [-842150451] * 6 and perm.dtype == p0.dtype and (p0 == -842150451).all()


def test_compaction_by_hand():
    alive = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1], bool)
    f, t0 = slab(16), np.full((ROWS, 16), 0xCDCDCDCD, "<u4")
    t, _, ends = BM.binned(f, t0, (~alive).astype(int), 12, 2, 1, 0, 1)
    assert ends.tolist() == [6, 12]
    assert np.array_equal(t[:9, :6], f[:9][:, [0, 3, 4, 6, 10, 11]]) and np.array_equal(t[14:, :6], f[14:][:, [0, 3, 4, 6, 10, 11]])
    assert (t[9:14] == 0xCDCDCDCD).all() and (t[:, 6:] == 0xCDCDCDCD).all()


def test_nothing_and_everything_dropped():
    f, t0 = slab(8), np.full((ROWS, 8), 0xCDCDCDCD, "<u4")
    t, _, ends = BM.binned(f, t0, np.zeros(0, int), 0, 3, 2, 1, 1)
    assert np.array_equal(t, t0) and ends.tolist() == [0, 0, 0]
    t, _, ends = BM.binned(f, t0, np.full(5, 2), 5, 3, 2, 1, 1)
    assert np.array_equal(t, t0) and ends.tolist() == [0, 0, 5]


def test_slot_terms_by_hand():
    # blocks of four: | 2 0 3 1 | 0 2 2 3 | 0 1 2 0 |
    begin, earlier, rank = BM.slot_decomposition(KEYS, 12, 4, block=4)
    assert begin.tolist() == [6, 0, 10, 4, 0, 6, 6, 10, 0, 4, 6, 0]
    assert earlier.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 1, 3, 2]
    assert rank.tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    slot = np.empty(12, int); slot[ORDER] = np.arange(12)
    assert (begin + earlier + rank).tolist() == slot.tolist()


@pytest.mark.parametrize("num_bins", [2, 3, 10, 64, 65, 1024, 1025])
def test_slot_terms_add_up_to_the_stable_position(num_bins):
    """On every key pattern of the device test, with blocks of 32 rays and waves of 8, at the stream sizes around them."""
    rng = np.random.default_rng(num_bins)
    for n in (1, 7, 8, 9, 31, 32, 33, 32 + 8, 32 + 9, 32 + 25, 65, 3 * 32 + 11):
        for name, keys in BM.key_patterns(n, num_bins, rng, block=32, wave=8).items():
            assert len(keys) == n and keys.min() >= 0 and keys.max() < num_bins, name
            begin, earlier, rank = BM.slot_decomposition(keys, n, num_bins, block=32)
            slot = np.empty(n, np.int64); slot[BM.stable_order(keys)] = np.arange(n)
            assert np.array_equal(begin + earlier + rank, slot), (n, name)
            _, perm, ends = BM.binned(None, None, keys, n, num_bins, num_bins, 1, 1, np.full(n + 3, -1, "<i4"))
            assert np.array_equal(perm[:n][slot], np.arange(n)) and (perm[n:] == -1).all() and ends[-1] == n


def test_patterns_hold_what_they_are_for():
    rng = np.random.default_rng(0)
    p = BM.key_patterns(2 * 1024 + 300, 65, rng)
    wave = lambda k, w: k[w * 64:(w + 1) * 64]
    assert len(np.unique(wave(p["i mod bins"], 3))) == 64
    assert len(np.unique(wave(p["one key per wave"], 3))) == 1 and p["one key per wave"][63] != p["one key per wave"][64]
    assert p["one key per half wave"][31] != p["one key per half wave"][32]
    k = p["a key only in the final block"]
    assert (k[:2048] == 0).all() and (k[2048:] == 32).any()
    assert set(np.unique(p["first and last key only"])) == {0, 64}
    assert np.bincount(p["skewed random"], minlength=65)[0] > 10 * np.bincount(p["skewed random"], minlength=65)[40]
