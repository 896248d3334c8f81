"""tests/collapse_bounded_model.py (the CPU model of rodent_hip_collapse_bvh2_tri1_bounded) against the "Stack limit" rules of
include/rodent_build.h, and the host-side refusals of the bounded entries.

Fixtures: the soup trees of test_collapse_model.py, the golden Cornell BVH2, its hand-made trees, and the bushy spine: a chain of D
nodes with a balanced bush of K leaves at every one, which the collapse without a limit takes past 63 entries.  For both widths and
the limits L in {H(0), H(0) + 4, 40, 63, the unbounded B} (those within [0, 63]):
* L = 0, and every L >= the unbounded B, give collapse_model.collapse's bytes;
* B and H(0) are recomputed top-down by walks written here (B from the wide nodes alone, H(0) from the BVH2): info[3] is that B, and
  B <= max(L, H(0));
* the model's bytes equal the rule stated once more node by node, in plain Python;
* every record lies in exactly one packet, every filled slot's bounds are a bit copy of the BVH2 slot it names;
* refit_wide_model.refit of a bounded collapse with the tree's own vertices keeps every byte;
* the oracle names the same triangles on the bounded tree as on the BVH2, and no stack passes B;
* the bounded entries refuse bad arguments with their codes, in their order.
The fixtures and cases() are also what tests/test_gpu_collapse_bounded.py runs on the device.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import collapse_bounded_model as BM
import collapse_model as M
import refit_model as R
import refit_wide_model as W
import test_collapse_model as T
from rodent_amd import formats as F

WIDTHS = (4, 8)
INF = np.float32(np.inf)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------

def bushy_spine_children(D, K):
    """Child pairs and leaf count of the bushy spine, numbered in pre-order: D spine nodes, child 0 of each a balanced subtree over K
    leaves of 3 records (k leaves split into k // 2 and the rest), child 1 the next spine node; the last one's child 1 is one more
    bush."""
    children, leaves = [], [0]

    def bush(k):
        """The reference of a subtree over k leaves, its nodes appended in pre-order."""
        if k == 1:
            leaves[0] += 1
            return ~(3 * (leaves[0] - 1))
        i = len(children)
        children.append(None)
        left = bush(k // 2)
        children[i] = [left, bush(k - k // 2)]
        return i + 1

    for d in range(D):
        i = len(children)
        children.append(None)
        left = bush(K)
        children[i] = [left, len(children) + 1 if d < D - 1 else bush(K)]
    return children, leaves[0]


def bushy_spine(D, K, seed=0):
    """(nodes, tris): the bushy spine with seeded random slot boxes, lo in [0, 1)^3 and extent in [0.1, 2)^3."""
    children, leaves = bushy_spine_children(D, K)
    nodes, tris = T.hand_tree(children, T.three_per_leaf(leaves))
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.0, 1.0, (len(nodes), 2, 3)).astype(np.float32)
    hi = lo + rng.uniform(0.1, 2.0, (len(nodes), 2, 3)).astype(np.float32)
    b = nodes["bounds"].reshape(-1, 2, 6)
    b[:, :, 0::2], b[:, :, 1::2] = lo, hi
    return nodes, tris


def spine_over_soup(D, K, seed):
    """(vertices, indices, nodes, tris): the bushy spine's topology over a plain soup, made a valid hierarchy by refit_model.refit: its
    record p holds triangle p."""
    children, leaves = bushy_spine_children(D, K)
    v, ix = T.plain_soup(3 * leaves, seed)
    nodes, tris = T.hand_tree(children, T.three_per_leaf(leaves))
    nodes, tris, info = R.refit(nodes, tris, v, ix)
    assert info.tolist() == [len(nodes), len(tris), 0, 0]
    return v, ix, nodes, tris


def fixtures():
    """(name, vertices, indices, nodes, tris); vertices and indices are None for the hand-made trees and for Cornell's host tree."""
    yield from T.soup_trees()
    yield ("cornell", None, None, *T.golden_cornell())
    yield ("hand", None, None, *T.sound_hand_tree())
    yield ("chain65", None, None, *T.deep_chain(65))
    yield ("spine20", None, None, *bushy_spine(20, 8))
    yield ("spine40", None, None, *bushy_spine(40, 8))


# ---- the walks written here ----------------------------------------------------------------------------------------------------

def small_flags(nodes, tris):
    return [T.is_small(nodes, tris, i) for i in range(len(nodes))]


def height_of_input(nodes, small):
    """H(0) top-down over the BVH2: the most inner nodes that are not small on a path from the root (0 when node 0 is small)."""
    best, todo = 0, [(0, 1)] if not small[0] else []
    while todo:
        i, h = todo.pop()
        best = max(best, h)
        todo += [(int(c) - 1, h + 1) for c in nodes["child"][i] if c > 0 and not small[c - 1]]
    return best


def bound_of_output(out):
    """B top-down from the wide nodes alone."""
    best, todo = 0, [(0, 0)]
    while todo:
        w, above = todo.pop()
        total = above + int((out["child"][w] != 0).sum()) - 1
        best = max(best, total)
        todo += [(int(c) - 1, total) for c in out["child"][w] if c > 0]
    return best


def limits(h0, unbounded):
    return sorted(L for L in {h0, h0 + 4, 40, 63, unbounded} if 0 <= L <= 63)


class Case:
    """One fixture: its tree, its small flags, H(0), and per width the unbounded collapse and the bounded ones by L (made on demand, once)."""

    def __init__(self, name, v, ix, nodes, tris):
        self.name, self.v, self.ix, self.nodes, self.tris = name, v, ix, nodes, tris
        self.small = small_flags(nodes, tris)
        self.h0 = height_of_input(nodes, self.small)
        self.unbounded = {w: M.collapse(w, nodes, tris) for w in WIDTHS}
        self._bounded = {}

    def limits(self, width):
        return limits(self.h0, int(self.unbounded[width][2][3]))

    def bounded(self, width, L):
        if (width, L) not in self._bounded:
            self._bounded[width, L] = BM.collapse(width, self.nodes, self.tris, L)
        return self._bounded[width, L]


def cases():
    return [Case(*f) for f in fixtures()]


@pytest.fixture(scope="module")
def all_cases():
    return cases()


# ---- the rule once more, node by node --------------------------------------------------------------------------------------------

def reference(width, nodes, tris, small, L):
    """The bounded collapse by recursion, as test_collapse_model.reference states the unbounded one:
    ([(root, [(ref, box)])] by ascending root, [(records, last)] by ascending first record, B)."""
    sys.setrecursionlimit(10000)
    box = nodes["bounds"].reshape(-1, 2, 6)
    child = nodes["child"]
    wide, packets, bound = [], [], [0]
    is_open = lambda ref: ref > 0 and not small[ref - 1]
    memo = {}

    def H(i):
        if i not in memo:
            memo[i] = 1 + max(H(int(c) - 1) if is_open(c) else 0 for c in child[i])
        return memo[i]

    def h(ref):
        return H(ref - 1) if is_open(ref) else 0

    def leaf(ref):
        if ref < 0:
            run = T.run_of(tris, ~ref)
            for q in range(0, len(run), 4):
                packets.append((run[q:q + 4], q + 4 >= len(run)))
        else:
            packets.append(([p for run in T.runs_below(nodes, tris, ref) for p in run], True))

    def grow(r, S):
        slots = [(int(child[r][k]), box[r][k]) for k in range(2) if child[r][k] != 0]
        while len(slots) < width:
            f = len(slots)
            best, top = -1, np.float32(-1)
            for j, (ref, b) in enumerate(slots):
                if not is_open(ref):
                    continue
                if L > 0 and any(S + f + h(other) > L for s, (other, _) in enumerate(slots) if s != j):
                    continue
                if T.area(b) > top:
                    best, top = j, T.area(b)
            if best < 0:
                break
            m = slots[best][0] - 1
            slots[best] = (int(child[m][0]), box[m][0])
            slots.append((int(child[m][1]), box[m][1]))
        wide.append((r, slots))
        bound[0] = max(bound[0], S + len(slots) - 1)
        for ref, _ in slots:
            if is_open(ref):
                grow(ref - 1, S + len(slots) - 1)
            else:
                leaf(ref)
    if small[0]:
        b = box[0]
        u = np.empty(6, np.float32)
        with np.errstate(all="ignore"):
            u[0::2], u[1::2] = np.fmin(b[0][0::2], b[1][0::2]), np.fmax(b[0][1::2], b[1][1::2])
        wide.append((0, [(1, u)]))
        leaf(1)
    else:
        grow(0, 0)
    return sorted(wide, key=lambda w: w[0]), sorted(packets, key=lambda p: p[0][0]), bound[0]


def reference_bytes(width, nodes, tris, small, L):
    """reference() written out as records."""
    wide, packets, bound = reference(width, nodes, tris, small, L)
    wide_id = {r: k for k, (r, _) in enumerate(wide)}
    packet_at = {p[0][0]: k for k, p in enumerate(packets)}
    out = np.zeros(len(wide), M.NODE[width])
    out["bounds"][:, 0::2, :], out["bounds"][:, 1::2, :] = INF, -INF
    for k, (r, slots) in enumerate(wide):
        for j, (ref, b) in enumerate(slots):
            out["bounds"][k][:, j] = b
            if ref > 0 and not small[ref - 1]:
                out["child"][k][j] = wide_id[ref - 1] + 1
            else:
                out["child"][k][j] = ~packet_at[~ref if ref < 0 else T.runs_below(nodes, tris, ref)[0][0]]
    pk = np.zeros(len(packets), F.TRI4)
    pk["prim_id"] = -1
    for k, (records, last) in enumerate(packets):
        for j, p in enumerate(records):
            e1, e2 = tris["e1"][p], tris["e2"][p]
            with np.errstate(all="ignore"):
                n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            pk["v0"][k][:, j], pk["e1"][k][:, j], pk["e2"][k][:, j], pk["n"][k][:, j] = tris["v0"][p], e1, e2, n
            pk["prim_id"][k][j], pk["geom_id"][k][j] = tris["prim_id"][p] & 0x7FFFFFFF, tris["geom_id"][p]
        if last:
            pk["prim_id"][k][3] |= T.INT_MIN
    return out, pk, [len(wide), len(packets), 0, bound]


# ---- tests -----------------------------------------------------------------------------------------------------------------------

def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and list(a[2]) == list(b[2])


def test_the_bushy_spine_is_what_the_limit_is_for(all_cases):
    by_name = {c.name: c for c in all_cases}
    assert (len(by_name["spine20"].nodes), len(by_name["spine40"].nodes)) == (167, 327)
    assert (by_name["spine20"].h0, by_name["spine40"].h0) == (23, 43)
    for width in WIDTHS:
        assert by_name["spine40"].unbounded[width][2][3] > 63       # the precondition: without a limit it passes the kernels' stack
        assert by_name["spine40"].bounded(width, 63)[2][3] <= 63
        assert not same(by_name["spine40"].bounded(width, 63), by_name["spine40"].unbounded[width])
    changed = sum(not same(c.bounded(w, L), c.unbounded[w]) for c in all_cases for w in WIDTHS for L in c.limits(w))
    print(f"{sum(len(c.limits(w)) for c in all_cases for w in WIDTHS)} (tree, width, L) cases, the limit changes {changed}")
    assert changed > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_no_limit_and_a_limit_not_below_b_give_the_unbounded_bytes(all_cases, width):
    for c in all_cases:
        free = c.unbounded[width]
        assert same(BM.collapse(width, c.nodes, c.tris), free) and same(c.bounded(width, 0), free), c.name
        for L in c.limits(width):
            if L >= free[2][3]:
                assert same(c.bounded(width, L), free), (c.name, L)


@pytest.mark.parametrize("width", WIDTHS)
def test_b_is_within_the_guarantee(all_cases, width):
    for c in all_cases:
        assert c.h0 <= 65 and c.unbounded[width][2][3] >= c.h0 - (c.h0 > 0), c.name
        for L in c.limits(width):
            out, pk, info = c.bounded(width, L)
            B = bound_of_output(out)
            assert info[3] == B and info[2] == 0, (c.name, L)
            assert B <= max(L, c.h0), (c.name, L, B, c.h0)
            assert B <= c.unbounded[width][2][3] or L == 0, (c.name, L)


@pytest.mark.parametrize("width", WIDTHS)
def test_model_equals_the_rule_node_by_node(all_cases, width):
    for c in all_cases:
        for L in c.limits(width):
            r_out, r_pk, r_info = reference_bytes(width, c.nodes, c.tris, c.small, L)
            out, pk, info = c.bounded(width, L)
            assert info.tolist() == r_info, (c.name, L)
            assert out.tobytes() == r_out.tobytes() and pk.tobytes() == r_pk.tobytes(), (c.name, L)


@pytest.mark.parametrize("width", WIDTHS)
def test_records_once_and_bounds_bit_copied(all_cases, width):
    for c in all_cases:
        box = c.nodes["bounds"].reshape(-1, 2, 6)
        named = {}                                                # the bytes of 6 stored bounds -> the child references stored with them
        for i, pair in enumerate(c.nodes["child"]):
            for k, ref in enumerate(pair):
                if ref != 0:
                    named.setdefault(box[i][k].tobytes(), []).append(int(ref))
        first_record = lambda ref: ~ref if ref < 0 else T.runs_below(c.nodes, c.tris, ref)[0][0]
        for L in c.limits(width):
            out, pk, info = c.bounded(width, L)
            assert info[0] == len(out) and info[1] == len(pk)
            # every record in exactly one lane: the valid lanes in packet order are the records in their order
            valid = W.valid_lanes(pk)
            assert int(valid.sum()) == len(c.tris), (c.name, L)
            for name in ("v0", "e1", "e2"):
                assert pk[name].transpose(0, 2, 1)[valid].tobytes() == c.tris[name].tobytes(), (c.name, L, name)
            assert (pk["prim_id"][valid] & 0x7FFFFFFF).tobytes() == (c.tris["prim_id"] & 0x7FFFFFFF).tobytes()
            assert pk["geom_id"][valid].tobytes() == c.tris["geom_id"].tobytes()
            if c.small[0]:
                continue                                          # one slot over the union of the root's boxes
            # a filled slot holds the bytes stored for a BVH2 reference of its kind: a leaf slot those of the packet leaf that starts at
            # its packet's first record, an inner slot those of an inner node that is not small
            starts = np.concatenate([[0], np.cumsum(valid.sum(1))])
            inner = 0
            for w in range(len(out)):
                for j in range(width):
                    ch = int(out["child"][w][j])
                    refs = named.get(out["bounds"][w][:, j].tobytes(), [])
                    if ch < 0:
                        assert any((r < 0 or c.small[r - 1]) and first_record(r) == starts[~ch] for r in refs), (c.name, L, w, j)
                    elif ch > 0:
                        inner += 1
                        assert any(r > 0 and not c.small[r - 1] for r in refs), (c.name, L, w, j)
            assert inner == len(out) - 1, (c.name, L)


@pytest.mark.parametrize("width", WIDTHS)
def test_refit_with_its_own_vertices_keeps_every_byte(all_cases, width):
    done = 0
    for c in all_cases:
        if c.v is None:
            continue
        for L in c.limits(width):
            out, pk, info = c.bounded(width, L)
            r_out, r_pk, r_info = W.refit(width, out, pk, c.v, c.ix)
            assert r_info.tolist() == [len(out), len(c.tris), 0, 0], (c.name, L)
            assert r_out.tobytes() == out.tobytes() and r_pk.tobytes() == pk.tobytes(), (c.name, L)
            done += 1
    assert done > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_oracle_names_the_same_triangles_as_on_the_bvh2(oracle, width):
    """On Cornell, on the trees of plain soups and on a bushy spine over a plain soup (no two triangles tie in t), at the limits that
    change the tree and at 63."""
    from rodent_amd import raygen
    trees = [("cornell", *T.golden_cornell())]
    trees += [(name, nodes, tris) for name, _, _, nodes, tris in T.soup_trees(T.plain_soup)]
    trees.append(("spine40-soup", *spine_over_soup(40, 8, 40)[2:]))
    changed = 0
    for name, nodes, tris in trees:
        small = small_flags(nodes, tris)
        h0, free = height_of_input(nodes, small), M.collapse(width, nodes, tris)
        corners = np.concatenate([tris["v0"], tris["v0"] - tris["e1"], tris["v0"] + tris["e2"]])
        rays = raygen.random_rays(corners.min(0), corners.max(0), 1024, 11, 0.0, 1.0)
        want, _ = oracle.traverse(2, nodes, tris, rays)
        for L in limits(h0, int(free[2][3])):
            out, pk, info = BM.collapse(width, nodes, tris, L)
            changed += not same((out, pk, info), free)
            got, st = oracle.traverse(width, out, pk, rays, algo="gpu")
            assert st["max_stack"] - 1 <= info[3] <= max(L, h0), (name, L)
            assert np.array_equal(got["tri_id"], want["tri_id"]), (name, L)
    assert changed > 0


# ---- symbols and refusals: no GPU is touched (dev = -1 is refused last) -------------------------------------------------------------

def test_symbols_are_exported_and_refusals_return_their_codes(native_build):
    from rodent_amd import abi, gpubuild
    l = abi.lib()
    names = ("rodent_hip_collapse_bounded_scratch_bytes", "rodent_hip_collapse_bvh2_tri1_bounded",
             "rodent_hip_collapse_bvh2_tri1_bounded_sync")
    assert all(n in abi.EXPORTS and getattr(l, n) for n in names)
    from conftest import ROOT
    header = (ROOT / "include" / "rodent_build.h").read_text()
    assert all(n + "(" in header for n in names) and "#define RODENT_BUILD_ERR_STACK_LIMIT -13" in header
    assert gpubuild.ERR_STACK_LIMIT == -13 and gpubuild.MAX_STACK_LIMIT == BM.MAX_STACK_LIMIT == 63
    sizes, old = l.rodent_hip_collapse_bounded_scratch_bytes, l.rodent_hip_collapse_scratch_bytes
    for width in WIDTHS:
        # two ints per node more, each array rounded up to the scratch alignment
        for nn, nt in ((1, 1), (5, 6), (142443, 283208)):
            assert 8 * nn <= sizes(width, nn, nt) - old(width, nn, nt) <= 8 * nn + 512
        assert sizes(width, 0, 1) == -1 and sizes(width, 1, 0) == -1 and sizes(width, -3, 5) == -1
    assert sizes(3, 5, 6) == -1 and sizes(2, 5, 6) == -1 and sizes(16, 5, 6) == -1 and sizes(0, 5, 6) == -1

    def call(width=4, limit=63, nodes=0x1000, nn=5, tris=0x2000, nt=6, wide=0x3000, packets=0x4000, scratch=0x5000, info=0x6000, dev=-1):
        return l.rodent_hip_collapse_bvh2_tri1_bounded(dev, width, limit, nodes, nn, tris, nt, wide, packets, scratch, info, None)
    assert call() == -5 and call(width=8) == -5 and call(limit=0) == -5 and call(limit=1) == -5     # nothing wrong but the device
    assert call(width=3) == -12 and call(width=3, limit=64) == -12 and call(width=2, limit=-1, nn=0) == -12
    assert call(limit=64) == -13 and call(limit=-1) == -13 and call(limit=1 << 20) == -13
    assert call(limit=64, nn=0) == -13 and call(limit=64, nodes=None) == -13 and call(limit=-1, nt=0, tris=None) == -13
    assert call(nn=0) == -11 and call(nt=0) == -11 and call(nn=0, tris=None) == -11
    for name in ("nodes", "tris", "wide", "packets", "scratch", "info"):
        assert call(**{name: None}) == -4, name
    host = (C.c_int32 * 4)(7, 7, 7, 7)
    sync = l.rodent_hip_collapse_bvh2_tri1_bounded_sync
    assert sync(-1, 3, 64, 0x1000, 5, 0x2000, 6, 0x3000, 0x4000, host) == -12
    assert sync(-1, 4, 64, 0x1000, 0, 0x2000, 6, 0x3000, 0x4000, host) == -13
    assert sync(-1, 4, -1, 0x1000, 5, 0x2000, 6, 0x3000, 0x4000, host) == -13
    assert sync(-1, 4, 63, 0x1000, 0, 0x2000, 6, 0x3000, 0x4000, host) == -11
    assert sync(-1, 8, 63, 0x1000, 5, 0x2000, 6, 0x3000, 0x4000, host) == -5
    assert list(host) == [7, 7, 7, 7]
