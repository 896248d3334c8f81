"""CPU model of the device collapse under a stack limit (rodent_hip_collapse_bvh2_tri1_bounded, rodent_amd/csrc/build_collapse.h).

collapse_model.py with the rules of include/rodent_build.h's "Stack limit" paragraph: H(i) = 1 + max(h(child 0), h(child 1)) for an inner
node that is not small, h(ref) = H(ref - 1) for an open reference and 0 otherwise; a wide node entered with S (the sum of (filled
slots - 1) over its ancestors) expands the slot of largest A among the open slots j with S + f + h(s) <= L for every other filled slot
s.  Then B <= max(L, H(0)).  stack_limit = 0 is collapse_model.collapse byte for byte.

Vectorised level by level like collapse_model, whose guards, small subtrees and A it imports; the growth and the records are restated
here.  heights() is the H of every node, for the tests.
"""
from __future__ import annotations

import numpy as np

from collapse_model import MAX_RUN, NODE, guards, half_area, small_subtrees
from rodent_amd import formats as F

F32 = np.float32
MAX_STACK_LIMIT = 63
NO_SLOT = -(1 << 20)              # the h of a slot that is not filled, below every sum: a slot without others passes whatever S


def open_refs(ref, small):
    """Which child references name an inner node that is not small (the guards have shown them sound)."""
    return (ref > 0) & (small[np.maximum(ref, 1) - 1] == 0)


def heights(child, levels, small):
    """H of every node: 0 for a small one."""
    H = np.zeros(len(child), np.int64)
    for level in reversed(levels):
        c = child[level]
        h = np.where(open_refs(c, small), H[np.maximum(c, 1) - 1], 0)
        H[level] = np.where(small[level] == 0, 1 + h.max(1), 0)
    return H


def grow_level(N, L, child, small, area, H, frontier, above):
    """All wide nodes rooted at `frontier`, entered with `above`, grown at once: (ref, src, count)."""
    R = len(frontier)
    rows, cols = np.arange(R), np.arange(N)
    ref, src, count = np.zeros((R, N), np.int64), np.zeros((R, N), np.int64), np.zeros(R, np.int64)
    for k in range(2):                                            # the root's children that are not 0, in order
        has = child[frontier, k] != 0
        ref[rows[has], count[has]] = child[frontier[has], k]
        src[rows[has], count[has]] = 2 * frontier[has] + k
        count += has
    for _ in range(N - 1):
        filled = cols < count[:, None]
        open_ = open_refs(ref, small) & filled
        a = area[src >> 1, src & 1]
        allowed = open_ & (a > F32(-1))                           # best = -1 and a strict >: a NaN never wins
        if L > 0:
            h = np.where(filled, np.where(open_, H[np.maximum(ref, 1) - 1], 0), NO_SLOT)
            at1 = np.argmax(h, axis=1)                            # the largest h, and the largest among the others
            h1 = h[rows, at1]
            rest = h.copy()
            rest[rows, at1] = NO_SLOT
            others = np.where(cols == at1[:, None], rest.max(1)[:, None], h1[:, None])
            allowed &= above[:, None] + count[:, None] + others <= L
        score = np.where(allowed, a, -np.inf)
        best = np.argmax(score, axis=1)                           # the first of equals
        grows = (score[rows, best] > -np.inf) & (count < N)
        g, b = rows[grows], best[grows]
        if not len(g):
            break
        m = ref[g, b] - 1
        ref[g, b], src[g, b] = child[m, 0], 2 * m
        ref[g, count[g]], src[g, count[g]] = child[m, 1], 2 * m + 1
        count[g] += 1
    return ref, src, count


def collapse(width, nodes, tris, stack_limit=0):
    """(wide nodes NODE4 | NODE8, packets TRI4, info int32[4]) as the device leaves them: info = [wide nodes, packets, flags, B]."""
    N, L = width, int(stack_limit)
    assert 0 <= L <= MAX_STACK_LIMIT
    info = np.zeros(4, np.int32)
    child = nodes["child"].astype(np.int64)
    flags, levels, run = guards(child, tris["prim_id"] < 0)
    if flags:
        info[2] = flags
        return np.zeros(0, NODE[N]), np.zeros(0, F.TRI4), info
    small, first = small_subtrees(child, levels, run)
    box = nodes["bounds"].reshape(-1, 2, 6)                       # [node, side]: the 6 bounds stored for that child
    if small[0]:
        # the whole tree is one packet under one slot
        ref = np.zeros((1, N), np.int64); ref[0, 0] = 1           # "node 0", read below as a small inner slot
        src = np.zeros((1, N), np.int64)
        roots, count, bound = np.zeros(1, np.int64), np.ones(1, np.int64), 0
    else:
        area, H = half_area(box), heights(child, levels, small)
        done, bound = [], 0
        frontier, above = np.zeros(1, np.int64), np.zeros(1, np.int64)
        while len(frontier):
            ref, src, count = grow_level(N, L, child, small, area, H, frontier, above)
            total = above + count - 1
            bound = max(bound, int(total.max()))
            done.append((frontier, ref, src, count))
            below = open_refs(ref, small) & (np.arange(N) < count[:, None])
            frontier, above = ref[below] - 1, np.repeat(total, below.sum(1))
        roots, ref, src, count = (np.concatenate(x) for x in zip(*done))
        order = np.argsort(roots, kind="stable")
        roots, ref, src, count = roots[order], ref[order], src[order], count[order]
    W = len(roots)
    filled = np.arange(N) < count[:, None]
    wide_id = np.full(len(nodes), -1, np.int64)
    wide_id[roots] = np.arange(W)
    # packets: one to a small subtree, ceil(k / 4) to a plain run; numbered by their first records
    below = np.maximum(ref, 1) - 1
    packed = filled & (ref > 0) & (small[below] > 0)
    plain = filled & (ref < 0)
    starts, lanes, lasts = [first[below[packed]]], [small[below[packed]]], [np.ones(int(packed.sum()), bool)]
    start, length = ~ref[plain], run[src >> 1, src & 1][plain]
    for q in range(0, MAX_RUN, 4):
        on = length > q
        starts.append(start[on] + q); lanes.append(np.minimum(4, length[on] - q)); lasts.append(length[on] <= q + 4)
    starts, lanes, lasts = np.concatenate(starts), np.concatenate(lanes), np.concatenate(lasts)
    order = np.argsort(starts, kind="stable")
    starts, lanes, lasts = starts[order], lanes[order], lasts[order]
    P = len(starts)
    packet_of = np.full(len(tris) + 1, -1, np.int64)
    packet_of[starts] = np.arange(P)
    packets = np.zeros(P, F.TRI4)
    ids = np.full((P, 4), -1, np.int32)
    geom = np.zeros((P, 4), np.int32)
    columns = {name: np.zeros((P, 3, 4), F32) for name in ("v0", "e1", "e2", "n")}
    with np.errstate(all="ignore"):
        for k in range(4):
            on = lanes > k
            rec = tris[starts[on] + k]
            e1, e2 = rec["e1"], rec["e2"]
            # n = e1 x e2, every product rounded on its own
            normal = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                               e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            for name, val in (("v0", rec["v0"]), ("e1", e1), ("e2", e2), ("n", normal)):
                columns[name][on, :, k] = val
            ids[on, k], geom[on, k] = rec["prim_id"] & 0x7FFFFFFF, rec["geom_id"]
    ids[lasts, 3] |= np.int32(-2 ** 31)
    for name, val in columns.items():
        packets[name] = val
    packets["prim_id"], packets["geom_id"] = ids, geom
    # node records
    out = np.zeros(W, NODE[N])
    bounds = np.empty((W, 6, N), F32)
    bounds[:, 0::2, :], bounds[:, 1::2, :] = np.inf, -np.inf
    if small[0]:
        b = box[0]
        bounds[0, 0::2, 0], bounds[0, 1::2, 0] = np.fmin(b[0, 0::2], b[1, 0::2]), np.fmax(b[0, 1::2], b[1, 1::2])
    else:
        w, j = np.nonzero(filled)
        bounds[w, :, j] = box[src[w, j] >> 1, src[w, j] & 1]
    wchild = np.zeros((W, N), np.int64)
    wchild[plain] = ~packet_of[~ref[plain]]
    wchild[packed] = ~packet_of[first[below[packed]]]
    inner = filled & (ref > 0) & ~packed
    wchild[inner] = wide_id[below[inner]] + 1
    out["bounds"], out["child"] = bounds, wchild.astype(np.int32)
    info[:] = [W, P, 0, bound]
    return out, packets, info
