"""CPU model of the device LBVH builder (rodent_amd/csrc/bvh_build.hip), stage for stage, in numpy.

It predicts the builder's output bytes: the same fp32 operations in the same order (numpy float32 arithmetic is correctly rounded,
like the kernels under -ffp-contract=off), the same stable order, the same Karras search.  Vectorised: Karras' searches run on all
nodes at once, the bottom-up pass level by level.  sort_references and emit work over references, so tests/trbvh_model.py and
tests/split_model.py share them; an unsplit build's references are its triangles (triangle_references).
"""
from __future__ import annotations

import numpy as np

from rodent_amd import formats as F

BAD_INDEX, NON_FINITE = 1, 2
F32 = np.float32


def _spread10(x):
    x = x.astype(np.uint32) & np.uint32(0x3FF)
    for shift, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):
        x = (x | (x << np.uint32(shift))) & np.uint32(mask)
    return x


def _clz32(x):
    """Leading zeros of uint32 values (x > 0)."""
    x = x.astype(np.uint64)
    n = np.zeros(x.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        small = x < (np.uint64(1) << np.uint64(32 - s))
        n = np.where(small, n + s, n)
        x = np.where(small, x << np.uint64(s), x)
    return n


def load_triangles(vertices, indices):
    """(corners [n, 3, 3] float32, geometry ids, flags): indices outside [0, nv) read as the origin."""
    vertices = np.asarray(vertices, F32).reshape(-1, 4)
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    nv = len(vertices)
    idx = indices[:, :3].astype(np.int64)
    ok = (idx >= 0) & (idx < nv)
    v = np.where(ok[..., None], vertices[np.where(ok, idx, 0), :3], F32(0))
    flags = 0
    if not ok.all():
        flags |= BAD_INDEX
    if not np.isfinite(vertices[np.where(ok, idx, 0), :3][ok]).all():
        flags |= NON_FINITE
    return v.astype(F32), indices[:, 3].copy(), flags


def boxes_of(V):
    """Boxes (lo_x hi_x lo_y hi_y lo_z hi_z) of triangles V [n, 3 vertices, 3 axes]."""
    b = np.empty((len(V), 6), F32)
    b[:, 0::2] = np.fmin(np.fmin(V[:, 0], V[:, 1]), V[:, 2])
    b[:, 1::2] = np.fmax(np.fmax(V[:, 0], V[:, 1]), V[:, 2])
    return b


def morton_codes(points):
    """30-bit codes of Morton points over their bounds (k_bounds + k_morton; fmin / fmax ignore NaN like fminf / fmaxf)."""
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(points, axis=0)
        hi = np.fmax.reduce(points, axis=0)
        extent = hi - lo
        scale = np.where((extent > 0) & np.isfinite(extent), F32(1024) / np.where(extent > 0, extent, F32(1)), F32(0)).astype(F32)
        q = (points - lo) * scale
        cell = np.fmin(np.fmax(q, F32(0)), F32(1023)).astype(np.uint32)
    return (_spread10(cell[:, 0]) << np.uint32(2)) | (_spread10(cell[:, 1]) << np.uint32(1)) | _spread10(cell[:, 2])


def triangle_references(v):
    """An unsplit build's references (reftri, refbox, points): triangle t is reference t, its box that of its corners x + 0 (-0 ->
    +0, as canon() in the kernel), its Morton point the centroid sum s = (v0 + v1) + v2."""
    with np.errstate(all="ignore"):
        return np.arange(len(v)), boxes_of(v + F32(0)), (v[:, 0] + v[:, 1]) + v[:, 2]


def sort_references(v, geom, reftri, refbox, points):
    """Morton codes, the sort and the leaves (k_morton ... k_leaves) over references: (codes, leaf boxes, Tri1 records without the
    end-of-leaf bits, prim ids) in (code, reference index) order, the stable radix sort's order."""
    codes = morton_codes(points)
    order = np.lexsort((np.arange(len(codes)), codes))
    tri = reftri[order]
    sv = v[tri]
    tris = np.zeros(len(tri), F.TRI1)
    with np.errstate(all="ignore"):
        tris["v0"] = sv[:, 0]
        tris["e1"] = sv[:, 0] - sv[:, 1]
        tris["e2"] = sv[:, 2] - sv[:, 0]
    tris["geom_id"] = geom[tri]
    return codes[order], refbox[order], tris, tri.astype(np.int64)


def single_leaf(box):
    """The one-node tree: child 0 the whole leaf, the empty slot as the host writer leaves it (+inf, -inf)."""
    nodes = np.zeros(1, F.NODE2)
    nodes[0]["bounds"][:6] = box
    nodes[0]["bounds"][6::2] = np.inf
    nodes[0]["bounds"][7::2] = -np.inf
    nodes[0]["child"] = [~0, 0]
    return nodes


def _delta(codes, i, j):
    n = len(codes)
    inside = (j >= 0) & (j < n)
    jj = np.where(inside, j, 0)
    a, b = codes[i], codes[jj]
    x = a ^ b
    out = np.where(x != 0, _clz32(np.where(x != 0, x, 1)), 32 + _clz32(np.where(i != jj, i ^ jj, 1)))
    return np.where(inside, out, -1)


def karras(codes):
    """Internal nodes 0 .. n-2: (first, last, split) of each (Karras 2012)."""
    n = len(codes)
    i = np.arange(n - 1, dtype=np.int64)
    d = np.where(_delta(codes, i, i + 1) > _delta(codes, i, i - 1), 1, -1)
    dmin = _delta(codes, i, i - d)
    lmax = np.full(len(i), 2, np.int64)
    grow = _delta(codes, i, i + lmax * d) > dmin
    while grow.any():
        lmax = np.where(grow, lmax * 2, lmax)
        grow = grow & (_delta(codes, i, i + lmax * d) > dmin)
    l = np.zeros(len(i), np.int64)
    t = lmax // 2
    while (t >= 1).any():
        act = t >= 1
        l = np.where(act & (_delta(codes, i, i + (l + t) * d) > dmin), l + t, l)
        t = t // 2
    j = i + l * d
    dnode = _delta(codes, i, j)
    s = np.zeros(len(i), np.int64)
    t = l.copy()
    act = np.ones(len(i), bool)
    while act.any():
        t = np.where(act, (t + 1) // 2, t)
        s = np.where(act & (_delta(codes, i, i + (s + t) * d) > dnode), s + t, s)
        act = act & (t > 1)
    split = i + s * d + np.minimum(d, 0)
    return np.minimum(i, j), np.maximum(i, j), split


def emit(codes, leafbox, tris, prim, max_leaf):
    """The hierarchy and its emission (k_karras ... k_emit / k_emit_root) over sorted references (sort_references): (nodes NODE2,
    tris TRI1, info int32[4] without the error flags)."""
    n = len(codes)
    tris = tris.copy()
    info = np.zeros(4, np.int32)
    last_in_leaf = np.zeros(n, bool)
    if n <= max_leaf:
        nodes = single_leaf(leafbox[0] if n == 1 else np.concatenate([np.fmin.reduce(leafbox[:, 0::2], 0)[:, None],
                                                                      np.fmax.reduce(leafbox[:, 1::2], 0)[:, None]], 1).reshape(-1))
        last_in_leaf[n - 1] = True
        info[0], info[1] = 1, 1
    else:
        first, last, split = karras(codes)
        m = n - 1
        size = last - first + 1
        kept = size > max_leaf
        newidx = np.where(kept, np.cumsum(kept) - 1, -1)
        single = [first == split, last == split + 1]
        child_ids = [split, split + 1]
        # levels top-down, then boxes and heights bottom-up one level at a time
        level = np.full(m, -1, np.int64)
        level[0] = 0
        frontier = np.array([0])
        while len(frontier):
            nxt = []
            for k in range(2):
                inner = frontier[~single[k][frontier]]
                level[child_ids[k][inner]] = level[inner] + 1
                nxt.append(child_ids[k][inner])
            frontier = np.concatenate(nxt)
        box = np.zeros((m, 6), F32)
        height = np.zeros(m, np.int64)
        for lv in range(level.max(), -1, -1):
            at = np.nonzero(level == lv)[0]
            cb, ch = [], []
            for k in range(2):
                c_ = child_ids[k][at]
                sg = single[k][at]
                cb.append(np.where(sg[:, None], leafbox[c_], box[np.where(sg, 0, c_)]))
                ch.append(np.where(sg, 0, height[np.where(sg, 0, c_)]))
            box[at, 0::2] = np.fmin(cb[0][:, 0::2], cb[1][:, 0::2])
            box[at, 1::2] = np.fmax(cb[0][:, 1::2], cb[1][:, 1::2])
            height[at] = np.where(kept[at], 1 + np.maximum(ch[0], ch[1]), 0)
        info[0], info[1] = int(kept.sum()), int(height[0])
        ks = np.nonzero(kept)[0]
        nodes = np.zeros(len(ks), F.NODE2)
        for k in range(2):
            c_ = child_ids[k][ks]
            sg = single[k][ks]
            cb = np.where(sg[:, None], leafbox[c_], box[np.where(sg, 0, c_)])
            inner = ~sg & kept[np.where(sg, 0, c_)]
            lo_k = first[ks] if k == 0 else split[ks] + 1
            hi_k = split[ks] if k == 0 else last[ks]
            nodes["bounds"][newidx[ks], 6 * k: 6 * k + 6] = cb
            nodes["child"][newidx[ks], k] = np.where(inner, newidx[np.where(sg, 0, c_)] + 1, ~lo_k)
            last_in_leaf[hi_k[~inner]] = True
    tris["prim_id"] = (prim | np.where(last_in_leaf, 1 << 31, 0)).astype(np.uint32).view(np.int32)
    return nodes, tris, info


def build(vertices, indices, max_leaf=2):
    """Returns (nodes NODE2, tris TRI1, info int32[4]) as the device builder writes them."""
    assert 1 <= max_leaf <= 8
    v, geom, flags = load_triangles(vertices, indices)
    assert 1 <= len(v) <= 1 << 25
    nodes, tris, info = emit(*sort_references(v, geom, *triangle_references(v)), max_leaf)
    info[2] = flags
    return nodes, tris, info


def depth_bound(n):
    return 30 + int(np.ceil(np.log2(n))) if n > 1 else 30


def sah_cost(nodes, tris, c_node=1.0, c_tri=1.0):
    """Surface-area cost of a BVH2 / Tri1 tree relative to its root box (for reports)."""
    def area(b):
        e = np.maximum(b[:, 1::2] - b[:, 0::2], 0)
        return 2 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    b = nodes["bounds"].astype(np.float64)
    root = np.concatenate([np.minimum(b[0, 0:6:2], b[0, 6:12:2])[:, None], np.maximum(b[0, 1:6:2], b[0, 7:12:2])[:, None]],
                          1).reshape(1, 6)
    root_area = max(area(root)[0], 1e-30)
    last = (tris["prim_id"] < 0)
    ends = np.nonzero(last)[0]
    cost = c_node * 1.0                                          # the root's node visit
    for k in range(2):
        c = nodes["child"][:, k]
        a = area(b[:, 6 * k: 6 * k + 6])
        used = c != 0
        a = np.where(used, a, 0)
        inner = c > 0
        cost += c_node * a[inner].sum() / root_area
        leaf = c < 0
        first = ~c[leaf]
        count = ends[np.searchsorted(ends, first)] - first + 1
        cost += c_tri * (a[leaf] * count).sum() / root_area
    return float(cost)
