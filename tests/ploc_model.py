"""CPU model of the device builder's PLOC topology stage (parallel locally-ordered clustering, Meister & Bittner 2018;
rodent_amd/csrc/build_ploc.h), in numpy, on top of tests/lbvh_model.py's sorted references and tests/trbvh_model.py's fit, treelet
passes and collapse.  It predicts the output bytes and info words of rodent_hip_build_bvh2_tri1_ploc: the rule of
include/rodent_build.h, the same fp32 operations in the same order, the same tie rules.

Vectorised: one iteration scans the 2 * radius offsets over all clusters at once.
"""
from __future__ import annotations

import numpy as np

import lbvh_model as L
import split_model as SP
import trbvh_model as T

F32 = np.float32
MAX_RADIUS, MAX_DEPTH = 64, 56
INFO_WORDS = 8


def clog2(x):
    """ceil(log2 x), clog2(1) = 0."""
    return int(x - 1).bit_length()


def nn_iterations(n):
    """I: the iterations that search nearest neighbours; later ones are forced."""
    return 4 * clog2(n) + 8


def cluster(leafbox, radius, depth_limit=0):
    """The clustering over the sorted references' boxes: (left, right, parent, iterations) of the explicit tree, ids 0 .. m-1 inner
    (node 0 the last merge), m + p the sorted reference p; parent has m + n entries (-1 for node 0)."""
    n = len(leafbox)
    m = n - 1
    D = depth_limit or MAX_DEPTH
    assert 1 <= radius <= MAX_RADIUS and clog2(n) <= D <= MAX_DEPTH
    I = nn_iterations(n)
    ids, box, h = m + np.arange(n, dtype=np.int64), np.array(leafbox, F32), np.zeros(n, np.int64)
    left, right, parent = np.zeros(m, np.int64), np.zeros(m, np.int64), np.full(m + n, -1, np.int64)
    t = 0
    while len(ids) > 1:
        C = len(ids)
        pos = np.arange(C, dtype=np.int64)
        if t < I:
            cap = D - clog2(C)
            bj, bd = np.full(C, -1, np.int64), np.zeros(C, F32)
            for o in [s * k for k in range(1, min(radius, C - 1) + 1) for s in (-1, 1)]:
                j = pos + o
                inside = (j >= 0) & (j < C)
                jj = np.where(inside, j, 0)
                with np.errstate(all="ignore"):
                    d = T.half_area(T.union(box, box[jj]))
                ok = inside & (1 + np.maximum(h, h[jj]) <= cap) & ~np.isnan(d)
                better = ok & ((bj < 0) | (d < bd) | ((d == bd) & ((pos ^ j) < (pos ^ bj))))
                bj, bd = np.where(better, j, bj), np.where(better, d, bd)
        else:
            bj = np.where((pos ^ 1) < C, pos ^ 1, -1)
        merged = (bj >= 0) & (bj[np.maximum(bj, 0)] == pos)
        lead = np.nonzero(merged & (pos < bj))[0]
        part = bj[lead]
        new = (C - 2) - np.arange(len(lead), dtype=np.int64)
        left[new], right[new] = ids[lead], ids[part]
        parent[ids[lead]], parent[ids[part]] = new, new
        box[lead] = T.union(box[lead], box[part])
        h[lead] = 1 + np.maximum(h[lead], h[part])
        ids[lead] = new
        keep = ~(merged & (pos > bj))
        ids, box, h = ids[keep], box[keep], h[keep]
        t += 1
    return left, right, parent, t


class Tree(T.Tree):
    """trbvh_model.Tree over the clustering's links instead of the Karras tree's."""

    def __init__(self, left, right, parent, leafbox, max_leaf, cn, ct):
        n = len(leafbox)
        m = n - 1
        self.n, self.m, self.max_leaf, self.cn, self.ct = n, m, max_leaf, F32(cn), F32(ct)
        self.left, self.right, self.parent = left.copy(), right.copy(), parent.copy()
        self.box = np.zeros((m + n, 6), F32)
        self.box[m:] = leafbox
        self.count = np.ones(m + n, np.int64)
        self.cost = np.zeros(m + n, F32)
        self.cost[m:] = (self.ct * T.half_area(leafbox)) * F32(1)
        self.height = np.zeros(m + n, np.int64)
        self.emitted = np.zeros(m + n, np.int64)
        self.rejected = 0


def emit_tree(t, srt, prim):
    """The tail's top-down emission (k_emit_opt_nodes / k_emit_opt_tris) of a fitted tree, as trbvh_model.emit ends:
    (nodes NODE2, tris TRI1, info int32[4] without the error flags)."""
    from rodent_amd import formats as F
    n, m = t.n, t.m
    idx, off, level = np.zeros(m + n, np.int64), np.zeros(m + n, np.int64), np.zeros(m + n, np.int64)
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
    if t.emitted[0] == 0:
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


def emit(codes, leafbox, srt, prim, max_leaf, passes, radius, depth_limit=0, node_cost=T.NODE_COST, tri_cost=T.TRI_COST,
         cluster_fn=cluster):
    """Clustering, fit, treelet passes, fit, emission over sorted references: (nodes, tris, info int32[4] without the flags,
    iterations).  One reference: the LBVH's single leaf."""
    n = len(codes)
    if n == 1:
        return (*L.emit(codes, leafbox, srt, prim, max_leaf), 0)
    t, iterations = fitted(leafbox, max_leaf, passes, radius, depth_limit, node_cost, tri_cost, cluster_fn)
    return (*emit_tree(t, srt, prim), iterations)


def fitted(leafbox, max_leaf, passes, radius, depth_limit=0, node_cost=T.NODE_COST, tri_cost=T.TRI_COST, cluster_fn=cluster):
    """(the tree after clustering, fit, the treelet passes and the last fit; iterations) over at least two sorted references."""
    left, right, parent, iterations = cluster_fn(leafbox, radius, depth_limit)
    t = Tree(left, right, parent, leafbox, max_leaf, node_cost, tri_cost)
    with np.errstate(all="ignore"):
        t.fit()
        for k in range(passes):
            t.treelet_pass(T.gamma(k))
        t.fit()
    return t, iterations


def root_cost(t):
    """A fitted tree's SAH cost: the root's cost over the root's half area."""
    return float(t.cost[0]) / float(T.half_area(t.box[0]))


def build(vertices, indices, max_leaf=2, passes=0, radius=16, depth_limit=0, budget=None, max_pieces=SP.MAX_PIECES,
          node_cost=T.NODE_COST, tri_cost=T.TRI_COST, cluster_fn=cluster):
    """Returns (nodes NODE2, tris TRI1, info int32[8]) as rodent_hip_build_bvh2_tri1_ploc writes them; `budget` None: no split
    options.  info[4] is the Tri1 count, info[7] the clustering's iterations."""
    assert 1 <= max_leaf <= 8 and 0 <= passes <= 3 and not (passes and depth_limit not in (0, MAX_DEPTH))
    info = np.zeros(INFO_WORDS, np.int32)
    if budget is None:
        v, geom, flags = L.load_triangles(vertices, indices)
        reftri, refbox, points = L.triangle_references(v)
    else:
        v, geom, flags, reftri, refbox, points, st = SP.references(vertices, indices, budget, max_pieces)
        info[5], info[6] = st["split"], st["unmade"]
    refs = L.sort_references(v, geom, reftri, refbox, points)
    nodes, tris, head, iterations = emit(*refs, max_leaf, passes, radius, depth_limit, node_cost, tri_cost, cluster_fn)
    info[:4] = head
    info[2], info[4], info[7] = flags, len(reftri), iterations
    return nodes, tris, info
