"""CPU model of the device builder's triangle pre-splitting (rodent_hip_build_bvh2_tri1_split, csrc/bvh_build.hip), stage for stage,
in numpy: frame, priority, allotment, the recursive cut, compaction and Morton points, then the stages of tests/lbvh_model.py
(sort_references, emit) or, with treelet passes, tests/trbvh_model.py (emit) over the references.
It predicts the output bytes: the same fp32 operations in the same order, the rules of include/rodent_build.h.

The cut runs in lock-step over all split triangles, one step of each triangle's loop per iteration, as the device's threads do.
"""
from __future__ import annotations

import numpy as np

import lbvh_model as L
import trbvh_model as T

F32 = np.float32
MAX_REFS = 1 << 25
MAX_PIECES = 64
MAX_BUDGET = 4.0
INFO_WORDS = 8


def triangle_flags(vertices, indices):
    """Per triangle: does it raise an error flag (an index outside the vertex array, a non-finite coordinate)?"""
    vertices = np.asarray(vertices, F32).reshape(-1, 4)
    idx = np.asarray(indices, np.int32).reshape(-1, 4)[:, :3].astype(np.int64)
    ok = (idx >= 0) & (idx < len(vertices))
    fin = np.isfinite(vertices[np.where(ok, idx, 0), :3]).all(-1)
    return ~(ok & fin).all(1)


def split_frame(tbox):
    """(lo[3], step[3]) of the plane grid; step 0: the axis has no planes."""
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(tbox[:, 0::2], 0).astype(F32)
        hi = np.fmax.reduce(tbox[:, 1::2], 0).astype(F32)
        step = (hi - lo) * F32(2.0 ** -10)
    step = np.where((step > 0) & np.isfinite(step), step, F32(0)).astype(F32)
    return lo, step


def find_plane(frame, b):
    """(level, axis, x) of the coarsest grid plane strictly inside each box b [k, 6], ties to x, y, z; level -1: none."""
    lo, step = frame
    k = len(b)
    best = np.full(k, -1, np.int64)
    axis = np.zeros(k, np.int64)
    x = np.zeros(k, F32)
    with np.errstate(all="ignore"):
        for a in range(3):
            if not step[a] > 0:
                continue
            c0, h0 = np.ones(k, np.int64), np.full(k, 1024, np.int64)
            c1, h1 = np.ones(k, np.int64), np.full(k, 1024, np.int64)
            for _ in range(10):
                m0, m1 = (c0 + h0) >> 1, (c1 + h1) >> 1
                g0 = lo[a] + m0.astype(F32) * step[a] > b[:, 2 * a]
                g1 = lo[a] + m1.astype(F32) * step[a] >= b[:, 2 * a + 1]
                a0, a1 = c0 < h0, c1 < h1
                h0, c0 = np.where(a0 & g0, m0, h0), np.where(a0 & ~g0, m0 + 1, c0)
                h1, c1 = np.where(a1 & g1, m1, h1), np.where(a1 & ~g1, m1 + 1, c1)
            cmin, cmax = c0, c1 - 1
            some = cmin <= cmax
            diff = np.where(some, (cmin - 1) ^ cmax, 1)
            level = np.floor(np.log2(diff.astype(np.float64))).astype(np.int64)    # highest set bit (exact for < 2^10)
            c = (cmax >> level) << level
            take = some & (level > best)
            best = np.where(take, level, best)
            axis = np.where(take, a, axis)
            x = np.where(take, lo[a] + c.astype(F32) * step[a], x).astype(F32)
    return best, axis, x


def priority(V, tbox, flagged, frame):
    level, _, _ = find_plane(frame, tbox)
    with np.errstate(all="ignore"):
        e, f = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        nx = e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1]
        ny = e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2]
        nz = e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]
        excess = np.fmax(F32(0), T.half_area(tbox) - F32(0.5) * ((np.abs(nx) + np.abs(ny)) + np.abs(nz)))
        p = np.sqrt(np.ldexp(F32(1), np.maximum(level, 0)).astype(F32) * excess).astype(F32)
    p = np.where((level >= 0) & ~flagged & np.isfinite(p), p, F32(0)).astype(F32)
    return p


def split_budget(n, budget):
    """B = min(floor(budget * n), 2^25 - n), budget a float32."""
    return min(int(np.floor(np.float64(F32(budget)) * n)), MAX_REFS - n)


def max_refs(n, budget, max_pieces):
    return n + min(split_budget(n, budget), n * (max_pieces - 1))


def allot(p, B, max_pieces):
    """(w, W, s): integer weights, their sum, extra pieces per triangle."""
    pmax = p.max() if len(p) else F32(0)
    with np.errstate(all="ignore"):
        w = np.floor((p / pmax) * F32(65536)).astype(np.uint64) if pmax > 0 else np.zeros(len(p), np.uint64)
    W = int(w.sum())
    if W == 0:
        return w, W, np.zeros(len(p), np.int64)
    s = np.minimum(np.uint64(max_pieces - 1), (w * np.uint64(B)) // np.uint64(W)).astype(np.int64)
    return w, W, s


def cut(V, B, axis, x):
    """The SBVH reference split of pieces B [k, 6] of triangles V [k, 3, 3] at planes (axis, x): boxes L, R [k, 6]."""
    k = len(B)
    rows = np.arange(k)
    Lb = np.tile(np.array([np.inf, -np.inf] * 3, F32), (k, 1))
    Rb = Lb.copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            P, Q = V[:, i], V[:, (i + 1) % 3]
            pa, qa = P[rows, axis], Q[rows, axis]
            for side, into in ((Lb, pa <= x), (Rb, pa >= x)):
                side[:, 0::2] = np.where(into[:, None], np.fmin(side[:, 0::2], P), side[:, 0::2])
                side[:, 1::2] = np.where(into[:, None], np.fmax(side[:, 1::2], P), side[:, 1::2])
            cross = ((pa < x) & (qa > x)) | ((pa > x) & (qa < x))
            t = (x - pa) / (qa - pa)
            for b in range(3):
                y = P[:, b] + t * (Q[:, b] - P[:, b])
                g = np.fmax(np.fmax(np.abs(P[:, b]), np.abs(Q[:, b])) * F32(2.0 ** -19), F32(2.0 ** -126))
                lo = np.fmax(y - g, np.fmin(P[:, b], Q[:, b]))
                hi = np.fmin(y + g, np.fmax(P[:, b], Q[:, b]))
                on = axis == b
                lo, hi = np.where(on, x, lo), np.where(on, x, hi)
                for side in (Lb, Rb):
                    side[:, 2 * b] = np.where(cross, np.fmin(side[:, 2 * b], lo), side[:, 2 * b])
                    side[:, 2 * b + 1] = np.where(cross, np.fmax(side[:, 2 * b + 1], hi), side[:, 2 * b + 1])
    for side in (Lb, Rb):
        side[:, 0::2] = np.fmax(side[:, 0::2], B[:, 0::2])
        side[:, 1::2] = np.fmin(side[:, 1::2], B[:, 1::2])
    Lb[rows, 2 * axis + 1] = np.fmin(Lb[rows, 2 * axis + 1], x)
    Rb[rows, 2 * axis] = np.fmax(Rb[rows, 2 * axis], x)
    return Lb, Rb


def _empty(b):
    return (b[:, 0] > b[:, 1]) | (b[:, 2] > b[:, 3]) | (b[:, 4] > b[:, 5])


def _longest(b):
    return np.fmax(np.fmax(b[:, 1] - b[:, 0], b[:, 3] - b[:, 2]), b[:, 5] - b[:, 4])


def split_pieces(V, tbox, s, frame):
    """Pieces of every triangle with s > 0: (boxes [total, 6] in slot order, first slot, pieces made, splits not made per triangle).
    Triangle t's slots are [first[t], first[t] + s[t]]: final pieces from the front, pending ones on a stack from the back."""
    n = len(V)
    first = np.concatenate([[0], np.cumsum(s + 1)[:-1]]).astype(np.int64)
    total = int((s + 1).sum())
    pbox = np.zeros((total, 6), F32)
    pk = np.zeros(total, np.int64)
    made = np.ones(n, np.int64)
    unmade = np.zeros(n, np.int64)
    ids = np.nonzero(s > 0)[0]
    if not len(ids):
        return pbox, first, made, unmade
    cb = tbox[ids].copy()
    k = s[ids].copy()
    out = np.zeros(len(ids), np.int64)
    sp = np.zeros(len(ids), np.int64)
    live = np.ones(len(ids), bool)
    fs, ss = first[ids], s[ids]
    for _ in range(4096):
        a = np.nonzero(live)[0]
        if not len(a):
            break
        level, axis, x = find_plane(frame, cb[a])
        final = (k[a] == 0) | (level < 0)
        c = a[~final]
        if len(c):
            Lb, Rb = cut(V[ids[c]], cb[c], axis[~final], x[~final])
            le, re = _empty(Lb), _empty(Rb)
            both = le & re
            final[np.nonzero(~final)[0][both]] = True
            one = le ^ re
            cb[c[one]] = np.where(le[one, None], Rb[one], Lb[one])
            two = ~le & ~re
            t2 = c[two]
            if len(t2):
                el, er = _longest(Lb[two]), _longest(Rb[two])
                with np.errstate(all="ignore"):
                    q = ((k[t2] - 1).astype(F32) * el) / (el + er)
                    kl = np.fmin(np.fmax(np.floor(q + F32(0.5)), F32(0)), (k[t2] - 1).astype(F32)).astype(np.int64)
                slot = fs[t2] + ss[t2] - sp[t2]
                pbox[slot] = Rb[two]
                pk[slot] = k[t2] - 1 - kl
                sp[t2] += 1
                cb[t2] = Lb[two]
                k[t2] = kl
        f = a[final]
        unmade[ids[f]] += k[f]
        pbox[fs[f] + out[f]] = cb[f] + F32(0)
        out[f] += 1
        done = sp[f] == 0
        live[f[done]] = False
        g = f[~done]
        sp[g] -= 1
        top = fs[g] + ss[g] - sp[g]
        cb[g] = pbox[top]
        k[g] = pk[top]
    assert not live.any(), "the cut loop did not end within its bound"
    made[ids] = out
    return pbox, first, made, unmade


def references(vertices, indices, budget, max_pieces):
    """(v raw [n,3,3], geom, flags, reftri, refbox, points, info words 4..6 as a dict, stage arrays)."""
    v, geom, flags = L.load_triangles(vertices, indices)
    n = len(v)
    with np.errstate(all="ignore"):
        V = (v + F32(0)).astype(F32)
    tbox = L.boxes_of(V)
    frame = split_frame(tbox)
    flagged = triangle_flags(vertices, indices)
    p = priority(V, tbox, flagged, frame)
    B = split_budget(n, budget)
    w, W, s = allot(p, B, max_pieces)
    pbox, first, made, unmade = split_pieces(V, tbox, s, frame)
    reftri = np.repeat(np.arange(n), made)
    dst = np.concatenate([[0], np.cumsum(made)[:-1]]).astype(np.int64)
    refbox = np.empty((len(reftri), 6), F32)
    points = np.empty((len(reftri), 3), F32)
    with np.errstate(all="ignore"):
        vsum = (v[:, 0] + v[:, 1]) + v[:, 2]
    uncut = s == 0
    refbox[dst[uncut]] = tbox[uncut]
    points[dst[uncut]] = vsum[uncut]
    cutt = np.nonzero(~uncut)[0]
    if len(cutt):
        src = np.concatenate([first[t] + np.arange(made[t]) for t in cutt])
        to = np.concatenate([dst[t] + np.arange(made[t]) for t in cutt])
        refbox[to] = pbox[src]
        with np.errstate(all="ignore"):
            points[to] = (pbox[src][:, 0::2] + pbox[src][:, 1::2]) * F32(1.5)
    stats = {"refs": len(reftri), "split": int((s > 0).sum()), "unmade": int(unmade.sum()), "B": B, "W": W, "s": s, "p": p,
             "w": w, "frame": frame, "tbox": tbox}
    return v, geom, flags, reftri, refbox, points, stats


def build(vertices, indices, max_leaf=2, passes=0, budget=0.0, max_pieces=MAX_PIECES, node_cost=T.NODE_COST, tri_cost=T.TRI_COST,
          stats=None):
    """Returns (nodes NODE2, tris TRI1, info int32[8]) as rodent_hip_build_bvh2_tri1_split writes them.  `stats`: a dict that
    receives the split stage's intermediate values."""
    assert 1 <= max_leaf <= 8 and 0 <= passes <= 3 and 0 <= budget <= MAX_BUDGET and 1 <= max_pieces <= MAX_PIECES
    v, geom, flags, reftri, refbox, points, st = references(vertices, indices, budget, max_pieces)
    if stats is not None:
        stats.update(st, reftri=reftri, refbox=refbox)
    refs = L.sort_references(v, geom, reftri, refbox, points)
    nodes, tris, head = T.emit(*refs, max_leaf, passes, node_cost, tri_cost) if passes else L.emit(*refs, max_leaf)
    info = np.zeros(INFO_WORDS, np.int32)
    info[:4] = head
    info[2], info[4], info[5], info[6] = flags, len(reftri), st["split"], st["unmade"]
    return nodes, tris, info


def check_split_structure(nodes, tris, num_tris, max_leaf, max_pieces, refbox_of=None, preorder=True):
    """trbvh_model.check_structure for a tree over references: indices in range, pre-order (inner child 0 at index + 1; preorder =
    False for the LBVH, numbered in Karras order), every node
    reached once, leaves of at most max_leaf contiguous records with the end bit on their last one only, every triangle id present
    at least once and at most max_pieces times, leaf boxes the union of their references' boxes (refbox_of: the box of every Tri1
    record, when known; else contained in the triangles' boxes), inner boxes exact unions of their children's.  Returns the depth,
    asserted to be at most 56."""
    nn, nt = len(nodes), len(tris)
    assert 1 <= nn <= max(1, nt - 1) and nt >= num_tris
    child = nodes["child"].astype(np.int64)
    bounds = nodes["bounds"]
    end = tris["prim_id"] < 0
    ids = (tris["prim_id"] & 0x7FFFFFFF).astype(np.int64)
    assert ((ids >= 0) & (ids < num_tris)).all()
    per = np.bincount(ids, minlength=num_tris)
    assert (per >= 1).all() and (per <= max_pieces).all()
    seen_node = np.zeros(nn, bool)
    seen_tri = np.zeros(nt, bool)
    depth = 0
    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        assert 0 <= i < nn and not seen_node[i], i
        assert d <= T.MAX_DEPTH, d
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
                assert 0 < j < nn and (k == 1 or j == i + 1 or not preorder), (i, k, c)
                stack.append((j, d + 1))
            else:
                f = ~c
                assert 0 <= f < nt
                e = f
                while not end[e]:
                    e += 1
                    assert e < nt and e - f < max_leaf, (f, e)
                assert not seen_tri[f: e + 1].any()
                seen_tri[f: e + 1] = True
                if refbox_of is not None:
                    rb = refbox_of[f: e + 1]
                    u = np.concatenate([np.fmin.reduce(rb[:, 0::2], 0)[:, None], np.fmax.reduce(rb[:, 1::2], 0)[:, None]], 1)
                    assert np.array_equal(u.reshape(-1), b), (i, k)
                else:
                    t = tris[f: e + 1]
                    v0 = t["v0"].astype(np.float64)
                    vs = np.stack([v0, v0 - t["e1"], v0 + t["e2"]]).reshape(-1, 3)
                    tol = 1e-5 * (1 + np.abs(vs).max())
                    assert (b[0::2] <= b[1::2]).all()
                    assert (b[0::2] >= vs.min(0) - tol).all() and (b[1::2] <= vs.max(0) + tol).all()
        for k in range(2):
            c = int(child[i, k])
            if c > 0:
                cb = bounds[c - 1]
                u = np.concatenate([np.fmin(cb[0:6:2], cb[6:12:2])[:, None], np.fmax(cb[1:6:2], cb[7:12:2])[:, None]], 1).reshape(-1)
                assert np.array_equal(u, bounds[i, 6 * k: 6 * k + 6]), (i, k)
    assert seen_node.all() and seen_tri.all()
    return depth


def leaf_boxes_of_records(nodes, tris):
    """Per Tri1 record: the box of the leaf holding it."""
    out = np.zeros((len(tris), 6), F32)
    end = tris["prim_id"] < 0
    for k in range(2):
        c = nodes["child"][:, k].astype(np.int64)
        for i in np.nonzero(c < 0)[0]:
            f = ~c[i]
            e = f
            while not end[e]:
                e += 1
            out[f: e + 1] = nodes["bounds"][i, 6 * k: 6 * k + 6]
    return out
