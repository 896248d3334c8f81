"""tests/collapse_model.py (the CPU model of rodent_hip_collapse_bvh2_tri1) against the rules of include/rodent_build.h, and the host-side
refusals of the collapse entries.

On the golden Cornell BVH2 and on lbvh_model / trbvh_model trees of seeded soups:
* the model's bytes equal a second statement of the rules, written here node by node (scalar, recursive) instead of level by level;
* top-down: every record is in exactly one lane, no small inner node is a wide root, every inner slot's box is the exact union of its
  child's slots, the numbering ascends, unused slots and lanes hold the stated bytes, B is recomputed from the wide tree alone;
* refit_wide_model.refit of a collapsed soup tree with the soup's own vertices keeps every byte;
* the oracle names the same triangle on the collapsed tree as on the BVH2;
* every malformed tree of the rules' list raises RODENT_BUILD_BAD_TOPOLOGY.
The trees and the malformed cases are also what tests/test_gpu_collapse.py runs on the device.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import collapse_model as M
import lbvh_model as L
import refit_wide_model as W
import trbvh_model as T
from rodent_amd import formats as F
from test_gpu_build import soup

WIDTHS = (4, 8)
SIZES = (1, 2, 3, 4, 5, 6, 63, 64, 65, 256, 257, 1000)
MAX_LEAVES = (1, 4, 8)
INT_MIN = np.int32(-2 ** 31)
INF = np.float32(np.inf)


def plain_soup(n, seed):
    """n small triangles over 3n vertices, none degenerate and no two alike: no two of them tie in t."""
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), np.float32)
    v[:, :3] = (rng.uniform(-50, 50, (n, 1, 3)) + rng.uniform(-4, 4, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


def soup_trees(make=soup):
    """(name, vertices, indices, BVH2 nodes, Tri1 records): LBVH trees with max_leaf 1, 4 and 8 and 3-pass treelet trees of the soups
    (test_gpu_build.soup: degenerate triangles, coincident pairs, a flat axis)."""
    for n in SIZES:
        for max_leaf in MAX_LEAVES:
            v, ix = make(n, n + max_leaf)
            yield (f"lbvh{max_leaf}-{n}", v, ix, *L.build(v, ix, max_leaf)[:2])
        v, ix = make(n, n + 4)
        yield (f"trbvh-{n}", v, ix, *T.build(v, ix, 4, 3)[:2])


@pytest.fixture(scope="module")
def trees():
    return list(soup_trees())


@pytest.fixture(scope="module")
def collapsed(trees):
    """{(name, width): the model's (nodes, packets, info)}: computed once, read by every test."""
    return {(name, w): M.collapse(w, nodes, tris) for name, _, _, nodes, tris in trees for w in WIDTHS}


# ---- the rules once more, node by node ---------------------------------------------------------------------------------------

def run_of(tris, s):
    e = s
    while tris["prim_id"][e] >= 0:
        e += 1
    return list(range(s, e + 1))


def runs_below(nodes, tris, ref):
    """The runs under a child reference, left to right."""
    if ref < 0:
        return [run_of(tris, ~ref)]
    out = []
    for c in nodes["child"][ref - 1]:
        if c != 0:
            out += runs_below(nodes, tris, int(c))
    return out


def is_small(nodes, tris, i):
    runs = runs_below(nodes, tris, i + 1)
    return sum(map(len, runs)) <= 4 and all(a[-1] + 1 == b[0] for a, b in zip(runs, runs[1:]))


def area(b):
    dx, dy, dz = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    return np.float32(np.float32(np.float32(dx * dy) + np.float32(dy * dz)) + np.float32(dz * dx))


def reference(width, nodes, tris):
    """The collapse by recursion: ([(root, [(ref, box)])] by ascending root, [(records, last)] by ascending first record, B)."""
    sys.setrecursionlimit(10000)
    small = [is_small(nodes, tris, i) for i in range(len(nodes))]
    box = nodes["bounds"].reshape(-1, 2, 6)
    wide, packets, bound = [], [], [0]

    def leaf(ref):
        if ref < 0:
            run = run_of(tris, ~ref)
            for q in range(0, len(run), 4):
                packets.append((run[q:q + 4], q + 4 >= len(run)))
        else:
            packets.append(([p for run in runs_below(nodes, tris, ref) for p in run], True))

    def grow(r, above):
        slots = [(int(nodes["child"][r][k]), box[r][k]) for k in range(2) if nodes["child"][r][k] != 0]
        while len(slots) < width:
            best, top = -1, np.float32(-1)
            for j, (ref, b) in enumerate(slots):
                if ref > 0 and not small[ref - 1] and area(b) > top:
                    best, top = j, area(b)
            if best < 0:
                break
            m = slots[best][0] - 1
            slots[best] = (int(nodes["child"][m][0]), box[m][0])
            slots.append((int(nodes["child"][m][1]), box[m][1]))
        wide.append((r, slots))
        bound[0] = max(bound[0], above + len(slots) - 1)
        for ref, _ in slots:
            if ref > 0 and not small[ref - 1]:
                grow(ref - 1, above + len(slots) - 1)
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
    return sorted(wide, key=lambda w: w[0]), sorted(packets, key=lambda p: p[0][0]), bound[0], small


def reference_bytes(width, nodes, tris):
    """reference() written out as records."""
    wide, packets, bound, small = reference(width, nodes, tris)
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
                out["child"][k][j] = ~packet_at[~ref if ref < 0 else runs_below(nodes, tris, ref)[0][0]]
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
            pk["prim_id"][k][3] |= INT_MIN
    return out, pk, [len(wide), len(packets), 0, bound], [r for r, _ in wide]


# ---- top-down checks of a collapsed tree ---------------------------------------------------------------------------------------

def assert_structure(width, nodes, tris, out, pk, info):
    """The properties the rules promise, read off the wide tree itself."""
    N = width
    assert info[0] == len(out) and info[1] == len(pk) and info[2] == 0
    # every record is in exactly one lane: the valid lanes in packet order are the records in their order
    valid = W.valid_lanes(pk)
    assert int(valid.sum()) == len(tris)
    for name in ("v0", "e1", "e2"):
        assert pk[name].transpose(0, 2, 1)[valid].tobytes() == tris[name].tobytes(), name
    assert (pk["prim_id"][valid] & 0x7FFFFFFF).tobytes() == (tris["prim_id"] & 0x7FFFFFFF).tobytes()
    assert pk["geom_id"][valid].tobytes() == tris["geom_id"].tobytes()
    # unused lanes: prim_id -1 and every other word 0; lanes are filled from the front
    assert (pk["prim_id"][~valid] == -1).all() and (pk["geom_id"][~valid] == 0).all()
    for name in ("v0", "e1", "e2", "n"):
        assert not pk[name].transpose(0, 2, 1)[~valid].view(np.uint32).any(), name
    assert valid[:, 0].all()
    # unused slots: child 0 with (+inf, -inf); slots are filled from the front; pad 0
    used = out["child"] != 0
    assert (used[:, :-1] >= used[:, 1:]).all() and not out["pad"].any()
    b = out["bounds"].transpose(0, 2, 1)[~used]
    assert (b[:, 0::2] == INF).all() and (b[:, 1::2] == -INF).all()
    # every wide node is named once, from node 0 down (a pre-order BVH2 gives ids above their parents', a Karras-ordered one need not)
    seen_nodes, leaf_starts, depth_sum = np.zeros(len(out), int), [], np.full(len(out), -1)
    depth_sum[0] = int(used[0].sum()) - 1
    todo = [0]
    while todo:
        w = todo.pop()
        for j in range(N):
            c = int(out["child"][w][j])
            if c > 0:
                seen_nodes[c - 1] += 1
                assert c > 1 and seen_nodes[c - 1] == 1
                depth_sum[c - 1] = depth_sum[w] + int(used[c - 1].sum()) - 1
                todo.append(c - 1)
                cb = out["bounds"][c - 1]                         # the slot's box is the exact union of the child's slots
                want = np.empty(6, np.float32)
                want[0::2], want[1::2] = np.fmin.reduce(cb[0::2], axis=1), np.fmax.reduce(cb[1::2], axis=1)
                assert out["bounds"][w][:, j].tobytes() == want.tobytes(), (w, j)
            elif c < 0:
                leaf_starts.append(~c)
    assert (seen_nodes[1:] == 1).all() and seen_nodes[0] == 0
    ends = pk["prim_id"][:, 3] < 0
    starts = np.sort(leaf_starts)
    assert len(np.unique(starts)) == len(starts) and starts[0] == 0 and ends[-1]
    assert np.array_equal(starts[1:], np.nonzero(ends)[0][:-1] + 1)          # every leaf starts behind the end of the one before
    assert info[3] == depth_sum.max()                             # B, from the wide tree alone


def golden_cornell():
    from conftest import GOLDEN
    return F.read_bvh(GOLDEN / "cornell.bvh", F.BVH2_TRI1)


@pytest.mark.parametrize("width", WIDTHS)
def test_model_equals_the_rules_node_by_node(trees, collapsed, width):
    cases = [(name, nodes, tris, collapsed[name, width]) for name, _, _, nodes, tris in trees]
    cn, ct = golden_cornell()
    cases.append(("cornell", cn, ct, M.collapse(width, cn, ct)))
    for name, nodes, tris, (out, pk, info) in cases:
        r_out, r_pk, r_info, roots = reference_bytes(width, nodes, tris)
        assert info.tolist() == r_info, name
        assert out.tobytes() == r_out.tobytes(), name
        assert pk.tobytes() == r_pk.tobytes(), name
        # no small inner node survives as a wide root (the root of a tree that is small as a whole is the one exception)
        assert roots == sorted(roots) and roots[0] == 0
        assert not any(is_small(nodes, tris, r) for r in roots[1:]), name
        assert_structure(width, nodes, tris, out, pk, info)
        if len(tris) <= 4:
            assert info.tolist() == [1, 1, 0, 0] and out["child"][0].tolist() == [~0] + [0] * (width - 1), name


@pytest.mark.parametrize("width", WIDTHS)
def test_refit_with_its_own_vertices_keeps_every_byte(trees, collapsed, width):
    for name, v, ix, nodes, tris in trees:
        out, pk, info = collapsed[name, width]
        r_out, r_pk, r_info = W.refit(width, out, pk, v, ix)
        assert r_info.tolist() == [len(out), len(tris), 0, 0], name
        assert r_out.tobytes() == out.tobytes(), name
        assert r_pk.tobytes() == pk.tobytes(), name


@pytest.mark.parametrize("width", WIDTHS)
def test_oracle_names_the_same_triangles_as_on_the_bvh2(oracle, trees, collapsed, width):
    """On Cornell and on the same trees of plain soups: the soups above hold coincident pairs, which tie in t, and which of a pair a ray
    is given depends on the order a layout tests them in.  On those every ray still meets a triangle in both layouts or in neither, and
    no stack passes B."""
    from rodent_amd import raygen
    cn, ct = golden_cornell()
    cases = [("cornell", cn, ct, M.collapse(width, cn, ct), True)]
    cases += [(name, nodes, tris, M.collapse(width, nodes, tris), True) for name, _, _, nodes, tris in soup_trees(plain_soup)]
    cases += [(name, nodes, tris, collapsed[name, width], False) for name, _, _, nodes, tris in trees]
    for name, nodes, tris, (out, pk, info), same_ids in cases:
        corners = np.concatenate([tris["v0"], tris["v0"] - tris["e1"], tris["v0"] + tris["e2"]])
        rays = raygen.random_rays(corners.min(0), corners.max(0), 1024, 11, 0.0, 1.0)
        want, _ = oracle.traverse(2, nodes, tris, rays)
        got, st = oracle.traverse(width, out, pk, rays, algo="gpu")
        assert st["max_stack"] - 1 <= info[3], name                # real entries (without the sentinel) against B
        if same_ids:
            assert np.array_equal(got["tri_id"], want["tri_id"]), name
        else:
            assert np.array_equal(got["tri_id"] < 0, want["tri_id"] < 0), name


# ---- malformed trees ---------------------------------------------------------------------------------------------------------------

def hand_tree(children, prims):
    """A BVH2 with these child pairs and Tri1 records with these prim words (geometry: record p is a triangle at x = 2p)."""
    nodes = np.zeros(len(children), F.NODE2)
    nodes["child"] = np.int32(children)
    nodes["bounds"][:, 0::2], nodes["bounds"][:, 1::2] = 0.0, 1.0
    tris = np.zeros(len(prims), F.TRI1)
    tris["v0"][:, 0] = 2.0 * np.arange(len(prims))
    tris["e1"][:, 1], tris["e2"][:, 2] = -1.0, 1.0
    tris["prim_id"] = np.int32(prims)
    return nodes, tris


def one_per_leaf(n):
    return [INT_MIN | np.int32(p) for p in range(n)]


def three_per_leaf(leaves):
    return [np.int32(p) | (INT_MIN if p % 3 == 2 else 0) for p in range(3 * leaves)]


def sound_hand_tree():
    """5 nodes, 6 leaves of 3 records: node 0 = (nodes 1, 2), node 1 = (nodes 3, 4), nodes 2, 3, 4 = two leaves each; every box is the
    unit cube, so the first slot wins every time."""
    return hand_tree([[2, 3], [4, 5], [~0, ~3], [~6, ~9], [~12, ~15]], three_per_leaf(6))


def malformed():
    """name -> (nodes, tris) for every case of the rules' list, 2 to 5 nodes each."""
    cases = {}
    n, t = sound_hand_tree()
    a = n.copy(); a["child"][1, 1] = 9
    cases["a child id out of range"] = (a, t)
    a = n.copy(); a["child"][4, 1] = 1
    cases["the root as a child"] = (a, t)
    a = n.copy(); a["child"][1, 1] = 4                           # node 3 twice, node 4 hangs in the air
    cases["a node named by two slots"] = (a, t)
    cases["a node that does not reach the root within 64 parents"] = deep_chain(66)
    a = n.copy(); a["child"][4, 1] = ~18
    cases["a leaf start beyond the records"] = (a, t)
    b = t.copy(); b["prim_id"][8] = 8                            # record 9 starts a leaf, record 8 does not end one
    cases["a leaf start whose predecessor has no end bit"] = (n, b)
    a = n.copy(); a["child"][4, 1] = ~12
    cases["a record held by two leaves"] = (a, t)
    a = n.copy(); a["child"][3, 1] = 0
    cases["an empty slot below the root"] = (a, t)
    prims = list(range(67)); prims[64] |= INT_MIN; prims[65] |= INT_MIN; prims[66] |= INT_MIN
    cases["a run longer than 64 records"] = hand_tree([[2, ~66], [~0, ~65]], prims)
    cases["a run that reaches the end of the records"] = hand_tree([[~0, 2], [~1, ~2]], [INT_MIN, INT_MIN | np.int32(1), 2, 3, 4, 5, 6, 7])
    return cases


def deep_chain(levels):
    """`levels` nodes one below the other, each with a leaf of one record: the last node is `levels - 1` parents from the root."""
    children = [[~i, i + 2] for i in range(levels - 1)] + [[~(levels - 1), ~levels]]
    return hand_tree(children, one_per_leaf(levels + 1))


@pytest.mark.parametrize("width", WIDTHS)
def test_malformed_trees_raise_the_flag(width):
    # width 4: the root grows into (leaf, node 2, node 4, leaf): 3 + 1 entries; width 8 takes the whole tree into one node of 6 slots
    out, pk, info = M.collapse(width, *sound_hand_tree())
    assert info.tolist() == {4: [3, 6, 0, 4], 8: [1, 6, 0, 5]}[width]
    assert out["child"][0].tolist() == {4: [~2, 2, 3, ~3], 8: [~2, ~0, ~4, ~3, ~1, ~5, 0, 0]}[width]
    for name, (nodes, tris) in malformed().items():
        assert M.collapse(width, nodes, tris)[2].tolist() == [0, 0, M.BAD_TOPOLOGY, 0], name
    # 64 parents are still a way to the root, 65 are not
    assert M.collapse(width, *deep_chain(65))[2][2] == 0
    assert M.collapse(width, *deep_chain(66))[2][2] == M.BAD_TOPOLOGY
    # a run of 64 records is still a run
    prims = list(range(64)); prims[63] |= INT_MIN
    out, pk, info = M.collapse(width, *hand_tree([[~0, ~64]], prims + [INT_MIN | np.int32(64)]))
    assert info.tolist() == [1, 17, 0, 1]


# ---- symbols and refusals: no GPU is touched (dev = -1 is refused last) -------------------------------------------------------------

def test_symbols_are_exported_and_refusals_return_their_codes(native_build):
    from rodent_amd import abi, gpubuild
    l = abi.lib()
    names = ("rodent_hip_collapse_scratch_bytes", "rodent_hip_collapse_bvh2_tri1", "rodent_hip_collapse_bvh2_tri1_sync")
    assert all(n in abi.EXPORTS and getattr(l, n) for n in names)
    from conftest import ROOT
    header = (ROOT / "include" / "rodent_build.h").read_text()
    assert all(n + "(" in header for n in names) and "#define RODENT_BUILD_ERR_WIDTH       -12" in header
    assert gpubuild.ERR_WIDTH == -12
    sizes = l.rodent_hip_collapse_scratch_bytes
    for width in WIDTHS:
        assert sizes(width, 1, 1) > 0 and sizes(width, 142443, 283208) > sizes(width, 1, 1)
        assert sizes(width, 0, 1) == -1 and sizes(width, 1, 0) == -1 and sizes(width, -3, 5) == -1
    assert sizes(3, 5, 6) == -1 and sizes(2, 5, 6) == -1 and sizes(16, 5, 6) == -1 and sizes(0, 5, 6) == -1

    def call(width=4, nodes=0x1000, nn=5, tris=0x2000, nt=6, wide=0x3000, packets=0x4000, scratch=0x5000, info=0x6000, dev=-1):
        return l.rodent_hip_collapse_bvh2_tri1(dev, width, nodes, nn, tris, nt, wide, packets, scratch, info, None)
    assert call() == -5 and call(width=8) == -5                   # nothing wrong but the device
    assert call(width=3) == -12 and call(width=2) == -12 and call(width=3, nn=0) == -12 and call(width=3, nodes=None) == -12
    assert call(nn=0) == -11 and call(nt=0) == -11 and call(nn=0, tris=None) == -11
    for name in ("nodes", "tris", "wide", "packets", "scratch", "info"):
        assert call(**{name: None}) == -4, name
    host = (C.c_int32 * 4)(7, 7, 7, 7)
    sync = l.rodent_hip_collapse_bvh2_tri1_sync
    assert sync(-1, 3, 0x1000, 5, 0x2000, 6, 0x3000, 0x4000, host) == -12
    assert sync(-1, 4, 0x1000, 0, 0x2000, 6, 0x3000, 0x4000, host) == -11
    assert sync(-1, 8, 0x1000, 5, 0x2000, 6, 0x3000, 0x4000, host) == -5
    assert list(host) == [7, 7, 7, 7]
