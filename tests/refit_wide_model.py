"""CPU model of the device refit of the wide layouts (rodent_hip_refit_bvh4_tri4 / _bvh8_tri4, rodent_amd/csrc/build_refit.h) in numpy.

It predicts the refitted bytes by the rules of include/rodent_build.h: the topology (child, pad, prim_id, geom_id) stays; every VALID
lane of a Tri4 packet (no -1 among prim_id[0 .. lane]) gets v0, e1 = v0 - v1, e2 = v2 - v0 and n = e1 x e2 of the moved triangle it
names, the other lanes keep their bytes; a packet's box is the union of its valid lanes' triangle boxes (corners taken as x + 0); a
leaf slot gets the union of its packets' boxes, an inner slot the union of its child's N slot boxes.  fp32 throughout, every product
of the cross product rounded on its own; min / max are exact, so the order they are taken in does not matter.  Vectorised like
refit_model.refit: lanes at once, leaves one packet position at a time, the climb one round of completed nodes at a time.

On a malformed tree the model raises the flags the device raises and completes no more nodes than it; WHICH of two slots naming one
node keeps it is the device's arrival order (here: the first in (node, slot) order), so bytes are only predicted for sound trees and
for trees whose two claims come from one node.
"""
from __future__ import annotations

import numpy as np

from lbvh_model import boxes_of, load_triangles
from refit_model import BAD_TOPOLOGY, deform  # noqa: F401  (deform: the tests' deformation, the same for every width)

F32 = np.float32
EMPTY = np.array([np.inf, -np.inf] * 3, F32)


def valid_lanes(tris):
    """[packets, 4] bool: lane k is valid when none of prim_id[0 .. k] is -1."""
    return np.logical_and.accumulate(tris["prim_id"] != -1, axis=1)


def refit(width, nodes, tris, vertices, indices):
    """(nodes NODE4 | NODE8, tris TRI4, info int32[4]) as the device leaves them: info = [nodes completed, lanes rewritten, flags, 0]."""
    N = width
    nodes, tris = nodes.copy(), tris.copy()
    assert nodes["child"].shape[1] == N
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    nn, npk, n = len(nodes), len(tris), len(indices)
    info = np.zeros(4, np.int32)
    flags = 0
    # lanes: the triangle prim_id & 0x7FFFFFFF of every valid lane, when the index table has it
    valid = valid_lanes(tris)
    prim = tris["prim_id"].view(np.uint32) & np.uint32(0x7FFFFFFF)
    ok = valid & (prim < n)
    if (valid & ~ok).any():
        flags |= BAD_TOPOLOGY
    pk, ln = np.nonzero(ok)
    V, _, tri_flags = load_triangles(vertices, indices[prim[ok]])
    flags |= tri_flags
    with np.errstate(all="ignore"):
        e1, e2 = V[:, 0] - V[:, 1], V[:, 2] - V[:, 0]
        normal = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                           e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                           e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        for name, val in (("v0", V[:, 0]), ("e1", e1), ("e2", e2), ("n", normal)):
            field = tris[name]
            field[pk, :, ln] = val
            tris[name] = field
        lanebox = np.tile(EMPTY, (npk, 4, 1))
        lanebox[pk, ln] = boxes_of(V + F32(0))
    pbox = np.empty((npk, 6), F32)
    pbox[:, 0::2] = np.fmin.reduce(lanebox[:, :, 0::2], axis=1)
    pbox[:, 1::2] = np.fmax.reduce(lanebox[:, :, 1::2], axis=1)
    info[1] = int(ok.sum())
    # leaf slots: packets ~child ... the first that ends its leaf (prim_id[3] < 0)
    child = nodes["child"].astype(np.int64)
    bounds = nodes["bounds"].copy()                              # [node, row, slot]
    ends = np.nonzero(tris["prim_id"][:, 3] < 0)[0]
    for k in range(N):
        c = child[:, k]
        leaf = np.nonzero(c < 0)[0]
        first = ~c[leaf]
        inside = first < npk
        if not inside.all():
            flags |= BAD_TOPOLOGY
        leaf, first = leaf[inside], first[inside]
        at = np.searchsorted(ends, first)
        ended = at < len(ends)
        if not ended.all():
            flags |= BAD_TOPOLOGY
        leaf, first = leaf[ended], first[ended]
        last = ends[at[ended]]
        acc = np.tile(EMPTY, (len(leaf), 1))
        step = 0
        while len(leaf) and (first + step <= last).any():
            on = first + step <= last
            pb = pbox[np.where(on, first + step, 0)]
            acc[:, 0::2] = np.where(on[:, None], np.fmin(acc[:, 0::2], pb[:, 0::2]), acc[:, 0::2])
            acc[:, 1::2] = np.where(on[:, None], np.fmax(acc[:, 1::2], pb[:, 1::2]), acc[:, 1::2])
            step += 1
        bounds[leaf, :, k] = acc
    # parent slots: every inner child is claimed once; ids out of range and the root are nobody's child
    parent = np.full(nn, -1, np.int64)
    for i, k in zip(*np.nonzero(child > 0)):
        c = child[i, k]
        if c > nn or c == 1 or parent[c - 1] != -1:
            flags |= BAD_TOPOLOGY
        else:
            parent[c - 1] = N * i + k
    # the climb: a node is complete after 1 + (children with id > 0) arrivals; a completed node hands its union to its parent slot
    needed = 1 + (child > 0).sum(1)
    arrivals = np.ones(nn, np.int64)
    front = np.nonzero(arrivals == needed)[0]
    done = 0
    while len(front):
        done += len(front)
        up = parent[front]
        front, up = front[up >= 0], up[up >= 0]
        b = bounds[front]
        u = np.empty((len(front), 6), F32)
        u[:, 0::2] = np.fmin.reduce(b[:, 0::2, :], axis=2)
        u[:, 1::2] = np.fmax.reduce(b[:, 1::2, :], axis=2)
        pn, slot = up // N, up % N
        bounds[pn, :, slot] = u
        np.add.at(arrivals, pn, 1)
        pn = np.unique(pn)
        front = pn[arrivals[pn] == needed[pn]]
    nodes["bounds"] = bounds
    info[0], info[2] = done, flags
    return nodes, tris, info


def contains(outer, inner):
    """Per node: every slot of `outer` (NODE4 | NODE8) contains that of `inner`; empty slots (+inf, -inf) contain nothing and are
    contained."""
    o, i = outer["bounds"], inner["bounds"]
    return ((o[:, 0::2] <= i[:, 0::2]) & (o[:, 1::2] >= i[:, 1::2])).all((1, 2))
