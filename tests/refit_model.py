"""CPU model of the device refit (rodent_hip_refit_bvh2_tri1, rodent_amd/csrc/build_refit.h) in numpy.

It predicts the refitted bytes: the topology (child, pad and w words) stays, every Tri1 record gets v0, e1 = v0 - v1, e2 = v2 - v0 of
the moved triangle it names, every leaf slot the union of its records' triangle boxes (corners taken as x + 0), every inner slot the
union of its child's two boxes.  fp32 throughout; min / max are exact, so the order they are taken in does not matter.  Vectorised:
leaves one record position at a time, the climb one round of completed nodes at a time.

On a malformed tree the model raises the flags the device raises and completes no more nodes than it; WHICH of two slots naming one
node keeps it is the device's arrival order (here: the first in (node, slot) order), so bytes are only predicted for sound trees.
"""
from __future__ import annotations

import numpy as np

from lbvh_model import boxes_of, load_triangles

BAD_TOPOLOGY = 4
F32 = np.float32
EMPTY = np.array([np.inf, -np.inf] * 3, F32)


def refit(nodes, tris, vertices, indices):
    """(nodes NODE2, tris TRI1, info int32[4]) as the device leaves them: info = [nodes completed, records rewritten, flags, 0]."""
    nodes, tris = nodes.copy(), tris.copy()
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    nn, nt, n = len(nodes), len(tris), len(indices)
    info = np.zeros(4, np.int32)
    flags = 0
    # records: the triangle prim_id & 0x7FFFFFFF, when the index table has it
    prim = tris["prim_id"].view(np.uint32) & np.uint32(0x7FFFFFFF)
    ok = prim < n
    if not ok.all():
        flags |= BAD_TOPOLOGY
    V, _, tri_flags = load_triangles(vertices, indices[prim[ok]])
    flags |= tri_flags
    with np.errstate(all="ignore"):
        for name, val in (("v0", V[:, 0]), ("e1", V[:, 0] - V[:, 1]), ("e2", V[:, 2] - V[:, 0])):
            field = tris[name]
            field[ok] = val
            tris[name] = field
        tribox = np.tile(EMPTY, (nt, 1))
        tribox[ok] = boxes_of(V + F32(0))
    info[1] = int(ok.sum())
    # leaf slots: records ~child ... the first with the end bit
    child = nodes["child"].astype(np.int64)
    bounds = nodes["bounds"].copy()
    ends = np.nonzero(tris["prim_id"] < 0)[0]
    for k in range(2):
        c = child[:, k]
        leaf = np.nonzero(c < 0)[0]
        first = ~c[leaf]
        inside = first < nt
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
            tb = tribox[np.where(on, first + step, 0)]
            acc[:, 0::2] = np.where(on[:, None], np.fmin(acc[:, 0::2], tb[:, 0::2]), acc[:, 0::2])
            acc[:, 1::2] = np.where(on[:, None], np.fmax(acc[:, 1::2], tb[:, 1::2]), acc[:, 1::2])
            step += 1
        bounds[leaf, 6 * k: 6 * k + 6] = acc
    # parent slots: every inner child is claimed once; ids out of range and the root are nobody's child
    parent = np.full(nn, -1, np.int64)
    for i, k in zip(*np.nonzero(child > 0)):
        c = child[i, k]
        if c > nn or c == 1 or parent[c - 1] != -1:
            flags |= BAD_TOPOLOGY
        else:
            parent[c - 1] = 2 * i + k
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
        u[:, 0::2] = np.fmin(b[:, 0:6:2], b[:, 6:12:2])
        u[:, 1::2] = np.fmax(b[:, 1:6:2], b[:, 7:12:2])
        pn, slot = up >> 1, up & 1
        for k in range(2):
            bounds[pn[slot == k], 6 * k: 6 * k + 6] = u[slot == k]
        np.add.at(arrivals, pn, 1)
        pn = np.unique(pn)
        front = pn[arrivals[pn] == needed[pn]]
    nodes["bounds"] = bounds
    info[0], info[2] = done, flags
    return nodes, tris, info


def deform(vertices, indices, seed, collapse=3):
    """The deformation of the refit tests and of scripts/bench_bvh_build.py --refit: a seeded smooth displacement (a sine wave per axis
    along another axis, amplitude 5 % of the mesh's extent) and `collapse` triangles collapsed to their first corner."""
    rng = np.random.default_rng(seed)
    v = np.array(vertices, F32).reshape(-1, 4).copy()
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    p = v[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    extent = max(float((hi - lo).max()), 1e-3)
    freq = rng.uniform(1.0, 3.0, 3) * 2 * np.pi / extent
    phase = rng.uniform(0, 2 * np.pi, 3)
    amp = 0.05 * extent * rng.uniform(0.5, 1.0, 3)
    for a in range(3):
        v[:, a] = (p[:, a] + amp[a] * np.sin(freq[a] * p[:, (a + 1) % 3] + phase[a])).astype(F32)
    for t in rng.choice(len(ix), min(collapse, len(ix)), replace=False):
        v[ix[t, 1], :3] = v[ix[t, 0], :3]
        v[ix[t, 2], :3] = v[ix[t, 0], :3]
    return v


def contains(outer, inner):
    """Per node: both slots of `outer` (NODE2) contain those of `inner`; empty slots (+inf, -inf) contain nothing and are contained."""
    o, i = outer["bounds"], inner["bounds"]
    return ((o[:, 0::2] <= i[:, 0::2]) & (o[:, 1::2] >= i[:, 1::2])).all(1)
