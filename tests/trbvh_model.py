"""CPU model of the device builder's optimisation stage (treelet restructuring + SAH leaf collapse, csrc/bvh_build.hip), stage for
stage, in numpy, on top of tests/lbvh_model.py's Morton codes and Karras tree.  It predicts the output bytes of
rodent_hip_build_bvh2_tri1_opt: the same fp32 operations in the same order, the same tie rules (include/rodent_build.h).

Vectorised: treelets are processed level by level in the order of their node's height at the start of the pass (nodes of equal
height have disjoint subtrees; the stored heights are true at the start of every pass, checked at its end), the DP runs over all 128 subsets of all treelets of a level as arrays.
"""
from __future__ import annotations

import numpy as np

import lbvh_model as L
from rodent_amd import formats as F

F32 = np.float32
TREELET = 7                     # treelet leaves
MAX_DEPTH = 56                  # Node2 levels the optimised tree may have (the host SBVH's cap)
NODE_COST, TRI_COST = 1.2, 1.0  # RODENT_BUILD_DEFAULT_NODE_COST / _TRI_COST


def gamma(pass_index):
    """Smallest subtree (in triangles) that gets a treelet in pass k (0-based): 7, 14, 28."""
    return TREELET << pass_index


def half_area(b):
    """(dx * dy + dy * dz) + dz * dx in fp32, boxes as lo_x hi_x lo_y hi_y lo_z hi_z."""
    dx, dy, dz = b[..., 1] - b[..., 0], b[..., 3] - b[..., 2], b[..., 5] - b[..., 4]
    return (dx * dy + dy * dz) + dz * dx


def union(a, b):
    out = np.empty(np.broadcast_shapes(a.shape, b.shape), F32)
    out[..., 0::2] = np.fmin(a[..., 0::2], b[..., 0::2])
    out[..., 1::2] = np.fmax(a[..., 1::2], b[..., 1::2])
    return out


# Static DP tables: subsets by size; for each subset S its candidate left parts P (the submasks of S holding S's lowest bit, S itself
# excluded) in increasing order -- the enumeration order the DP's first-minimum tie rule refers to.
_BY_SIZE = {s: [S for S in range(1, 128) if bin(S).count("1") == s] for s in range(1, 8)}
_CANDS = {}
for _S in range(1, 128):
    _low = _S & -_S
    _CANDS[_S] = np.array([_low | q for q in range(0, _S ^ _low) if (q & ~(_S ^ _low)) == 0], np.int64)
_POP = np.array([bin(S).count("1") for S in range(128)], np.int64)


class Tree:
    """Explicit binary tree: ids 0 .. m-1 internal (Karras numbering), m + p the sorted triangle p."""

    def __init__(self, first, last, split, leafbox, max_leaf, cn, ct):
        n = len(leafbox)
        m = n - 1
        self.n, self.m, self.max_leaf, self.cn, self.ct = n, m, max_leaf, F32(cn), F32(ct)
        self.left = np.where(first == split, m + split, split).astype(np.int64)
        self.right = np.where(last == split + 1, m + split + 1, split + 1).astype(np.int64)
        self.parent = np.full(m + n, -1, np.int64)
        self.parent[self.left] = np.arange(m)
        self.parent[self.right] = np.arange(m)
        self.box = np.zeros((m + n, 6), F32)
        self.box[m:] = leafbox
        self.count = np.ones(m + n, np.int64)
        self.cost = np.zeros(m + n, F32)
        self.cost[m:] = (self.ct * half_area(leafbox)) * F32(1)
        self.height = np.zeros(m + n, np.int64)
        self.emitted = np.zeros(m + n, np.int64)      # Node2 records in the subtree when the node is emitted (0: a leaf)
        self.rejected = 0

    def levels(self):
        """Internal nodes grouped by depth from the root (top-down), and every node's depth."""
        depth = np.full(self.m + self.n, -1, np.int64)
        depth[0] = 0
        out, frontier, d = [], np.array([0]), 0
        while len(frontier):
            out.append(frontier)
            kids = np.concatenate([self.left[frontier], self.right[frontier]])
            depth[kids] = d + 1
            frontier = kids[kids < self.m]
            d += 1
        return out, depth

    def fit(self):
        """Boxes, counts, heights, costs and emitted counts bottom-up (k_fit)."""
        levels, _ = self.levels()
        for at in reversed(levels):
            l, r = self.left[at], self.right[at]
            self.box[at] = union(self.box[l], self.box[r])
            self.count[at] = self.count[l] + self.count[r]
            col = self.refit(at)
            self.emitted[at] = np.where(col, 0, 1 + self.emitted[l] + self.emitted[r])

    def refit(self, at):
        """Height and cost of inner nodes `at` from their current children (box and count are already theirs); returns which
        nodes are collapsed."""
        l, r = self.left[at], self.right[at]
        self.height[at] = 1 + np.maximum(self.height[l], self.height[r])
        a = half_area(self.box[at])
        inner = self.cn * a + (self.cost[l] + self.cost[r])
        leafc = (self.ct * a) * self.count[at].astype(F32)
        col = (self.count[at] <= self.max_leaf) & (leafc <= inner)
        self.cost[at] = np.where(col, leafc, inner)
        return col

    def treelet_pass(self, g):
        _, depth = self.levels()
        h0 = self.height[: self.m].copy()
        ready = np.nonzero(self.count[: self.m] >= g)[0]
        for h in np.unique(h0[ready]):
            self._treelets(ready[h0[ready] == h], depth)
        # every stored height is true again (rejected treelets refit their roots): the next pass may order its batches by them
        inner = np.arange(self.m)
        assert np.array_equal(self.height[inner], 1 + np.maximum(self.height[self.left[inner]], self.height[self.right[inner]]))

    def _treelets(self, R, depth):
        T, m = len(R), self.m
        rows = np.arange(T)
        slots = np.full((T, TREELET), -1, np.int64)
        slots[:, 0], slots[:, 1] = self.left[R], self.right[R]
        expanded = np.zeros((T, TREELET - 2), np.int64)
        for e in range(TREELET - 2):
            k = 2 + e
            cand = slots[:, :k] < m
            a = np.where(cand, half_area(self.box[np.maximum(slots[:, :k], 0)]), -np.inf)
            best = np.argmax(a, axis=1)                               # the first slot of largest area
            c = slots[rows, best]
            expanded[:, e] = c
            slots[rows, best] = self.left[c]
            slots[:, k] = self.right[c]
        sbox = np.zeros((T, 128, 6), F32)
        cnt = np.zeros((T, 128), np.int64)
        cost = np.zeros((T, 128), F32)
        hgt = np.zeros((T, 128), np.int64)
        for i in range(TREELET):
            sbox[:, 1 << i] = self.box[slots[:, i]]
            cnt[:, 1 << i] = self.count[slots[:, i]]
            cost[:, 1 << i] = self.cost[slots[:, i]]
            hgt[:, 1 << i] = self.height[slots[:, i]]
        for S in range(3, 128):
            if _POP[S] > 1:
                low = S & -S
                sbox[:, S] = union(sbox[:, S ^ low], sbox[:, low])
                cnt[:, S] = cnt[:, S ^ low] + cnt[:, low]
        area = half_area(sbox)
        part = np.zeros((T, 128), np.int64)
        for s in range(2, TREELET + 1):
            for S in _BY_SIZE[s]:
                P = _CANDS[S]
                cand = cost[:, P] + cost[:, S ^ P]
                j = np.argmin(cand, axis=1)                           # the first candidate of least cost
                inner = self.cn * area[:, S] + cand[rows, j]
                leafc = (self.ct * area[:, S]) * cnt[:, S].astype(F32)
                cost[:, S] = np.where((cnt[:, S] <= self.max_leaf) & (leafc <= inner), leafc, inner)
                part[:, S] = P[j]
        # the new topology in pre-order (left part first): a stack of subsets
        full = (1 << TREELET) - 1
        topo = np.zeros((T, TREELET - 1), np.int64)
        stack = np.zeros((T, TREELET + 1), np.int64)
        stack[:, 0] = full
        sp = np.ones(T, np.int64)
        for j in range(TREELET - 1):
            sp -= 1
            S = stack[rows, sp]
            topo[:, j] = S
            P = part[rows, S]
            Q = S ^ P
            for X in (Q, P):                                          # pushed right first: the left part is popped next
                push = _POP[X] >= 2
                stack[rows[push], sp[push]] = X[push]
                sp = sp + push
        for j in range(TREELET - 2, -1, -1):
            S = topo[:, j]
            P = part[rows, S]
            hgt[rows, S] = 1 + np.maximum(hgt[rows, P], hgt[rows, S ^ P])
        accept = hgt[:, full] <= MAX_DEPTH - depth[R]
        self.rejected += int((~accept).sum())
        ids = np.full((T, 128), -1, np.int64)
        for i in range(TREELET):
            ids[:, 1 << i] = slots[:, i]
        ids[rows, topo[:, 0]] = R
        for j in range(1, TREELET - 1):
            ids[rows, topo[:, j]] = expanded[:, j - 1]
        a = rows[accept]
        for j in range(TREELET - 1):
            S = topo[a, j]
            P = part[a, S]
            node, l, r = ids[a, S], ids[a, P], ids[a, S ^ P]
            self.left[node], self.right[node] = l, r
            self.parent[l], self.parent[r] = node, node
            self.box[node] = sbox[a, S]
            self.count[node] = cnt[a, S]
            self.cost[node] = cost[a, S]
            self.height[node] = hgt[a, S]
        # a treelet kept as it is still gets its root's height and cost from its children, which this pass may have changed:
        # ancestors read them, both for their own DP and for the depth rule
        self.refit(R[~accept])


def emit(codes, leafbox, srt, prim, max_leaf, passes, node_cost=NODE_COST, tri_cost=TRI_COST):
    """The treelet passes, the collapse and the pre-order emission (k_explicit ... k_emit_opt_tris) over sorted references
    (lbvh_model.sort_references): (nodes NODE2, tris TRI1, info int32[4] without the error flags; info[3] counts the treelet
    topologies the depth rule rejected).  One reference: the LBVH's single leaf."""
    n = len(codes)
    if n == 1:
        return L.emit(codes, leafbox, srt, prim, max_leaf)
    first, last, split = L.karras(codes)
    t = Tree(first, last, split, leafbox, max_leaf, node_cost, tri_cost)
    with np.errstate(all="ignore"):
        t.fit()
        for k in range(passes):
            t.treelet_pass(gamma(k))
        t.fit()
    m = t.m
    # top-down: Node2 index, first triangle, level, and the topmost collapsed node above every node (itself included)
    idx = np.zeros(m + n, np.int64)
    off = np.zeros(m + n, np.int64)
    level = np.zeros(m + n, np.int64)
    top = np.full(m + n, -1, np.int64)
    levels, _ = t.levels()
    for at in levels:
        top[at] = np.where(top[at] >= 0, top[at], np.where(t.emitted[at] == 0, at, -1))
        l, r = t.left[at], t.right[at]
        idx[l], idx[r] = idx[at] + 1, idx[at] + 1 + t.emitted[l]
        off[l], off[r] = off[at], off[at] + t.count[l]
        level[l], level[r] = level[at] + 1, level[at] + 1
        top[l], top[r] = top[at], top[at]
    leaves = np.arange(m, m + n)
    top[leaves] = np.where(top[leaves] >= 0, top[leaves], leaves)
    info = np.zeros(4, np.int32)
    info[3] = t.rejected
    tris = np.zeros(n, F.TRI1)
    pos = off[leaves]
    last_in_leaf = pos == off[top[leaves]] + t.count[top[leaves]] - 1
    tris[pos] = srt
    tris["prim_id"][pos] = (prim | np.where(last_in_leaf, 1 << 31, 0)).astype(np.uint32).view(np.int32)
    if t.emitted[0] == 0:                                             # the root collapsed: the single-leaf form
        info[0], info[1] = 1, 1
        return L.single_leaf(t.box[0]), tris, info
    kept = np.nonzero((t.emitted[:m] > 0) & (top[:m] < 0))[0]
    nodes = np.zeros(int(t.emitted[0]), F.NODE2)
    for k, ch in enumerate((t.left[kept], t.right[kept])):
        nodes["bounds"][idx[kept], 6 * k: 6 * k + 6] = t.box[ch]
        inner = (ch < m) & (t.emitted[ch] > 0)
        nodes["child"][idx[kept], k] = np.where(inner, idx[ch] + 1, ~off[ch])
    info[0], info[1] = len(nodes), int(level[kept].max()) + 1
    return nodes, tris, info


def build(vertices, indices, max_leaf=2, passes=1, node_cost=NODE_COST, tri_cost=TRI_COST):
    """Returns (nodes NODE2, tris TRI1, info int32[4]) as rodent_hip_build_bvh2_tri1_opt writes them; info[3] counts the treelet
    topologies the depth rule rejected."""
    assert 1 <= max_leaf <= 8 and 0 <= passes <= 3
    if passes == 0:
        return L.build(vertices, indices, max_leaf)
    v, geom, flags = L.load_triangles(vertices, indices)
    nodes, tris, info = emit(*L.sort_references(v, geom, *L.triangle_references(v)), max_leaf, passes, node_cost, tri_cost)
    info[2] = flags
    return nodes, tris, info


def check_structure(nodes, tris, num_tris, max_leaf):
    """Host check of a BVH2 / Tri1 tree before anything traces it: every index in range, every node reached once in pre-order
    (inner child 0 at index + 1), every triangle in exactly one leaf of at most max_leaf contiguous records with the end bit on its
    last one only, inner boxes the exact union of their children's, leaf boxes tight around their triangles.  Returns the depth
    (Node2 levels), asserted to be at most MAX_DEPTH."""
    nn, nt = len(nodes), len(tris)
    assert nt == num_tris and 1 <= nn <= max(1, num_tris - 1)
    child = nodes["child"].astype(np.int64)
    bounds = nodes["bounds"]
    end = tris["prim_id"] < 0
    seen_node = np.zeros(nn, bool)
    seen_tri = np.zeros(nt, bool)
    depth = 0
    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        assert 0 <= i < nn and not seen_node[i], i
        assert d <= MAX_DEPTH, d
        seen_node[i] = True
        depth = max(depth, d)
        for k in range(2):
            c = int(child[i, k])
            b = bounds[i, 6 * k: 6 * k + 6]
            if c == 0:
                assert nn == 1 and k == 1 and np.isposinf(b[0::2]).all() and np.isneginf(b[1::2]).all()
                continue
            if c > 0:
                j = c - 1
                assert 0 < j < nn and (k == 1 or j == i + 1), (i, k, c)
                stack.append((j, d + 1))
            else:
                f = ~c
                assert 0 <= f < nt
                e = f
                while not end[e]:
                    e += 1
                    assert e < nt and e - f < max_leaf, (f, e)
                assert e - f + 1 <= max_leaf
                assert not seen_tri[f: e + 1].any()
                seen_tri[f: e + 1] = True
                t = tris[f: e + 1]
                v0 = t["v0"].astype(np.float64)
                vs = np.stack([v0, v0 - t["e1"], v0 + t["e2"]]).reshape(-1, 3)
                lo, hi = b[0::2].astype(np.float64), b[1::2].astype(np.float64)
                tol = 1e-5 * (1 + np.abs(vs).max())
                assert (vs.min(0) >= lo - tol).all() and (vs.max(0) <= hi + tol).all()
                assert np.allclose(vs.min(0), lo, atol=tol) and np.allclose(vs.max(0), hi, atol=tol)
        for k in range(2):                                       # an inner child's two slots union to the slot above
            c = int(child[i, k])
            if c > 0:
                cb = bounds[c - 1]
                u = np.concatenate([np.fmin(cb[0:6:2], cb[6:12:2])[:, None], np.fmax(cb[1:6:2], cb[7:12:2])[:, None]], 1).reshape(-1)
                assert np.array_equal(u, bounds[i, 6 * k: 6 * k + 6]), (i, k)
    assert seen_node.all() and seen_tri.all()
    assert sorted(tris["prim_id"] & 0x7FFFFFFF) == list(range(num_tris))
    return depth
