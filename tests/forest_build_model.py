"""CPU model of the forest build (rodent_hip_build_objects, rodent_amd/csrc/build_forest.h): lbvh_model.build per object, then the
packing of instances.pack_objects (instance_model.pack).  No arithmetic of its own.

Also the fixture objects of the forest build's tests, and three PERTURBED models, each a mistake the one-list form invites; the
fixtures are chosen so that each of them shows (tests/test_forest_build_model.py).
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import lbvh_model as L
import scene_update_model as SU
from rodent_amd import formats as F

F32 = np.float32


def build(vertices, indices, ranges, max_leaf=2):
    """(nodes NODE2, tris TRI1, table OBJECT, info int32 (K, 4)): every object of `ranges` ((first_tri, num_tris) rows of the
    concatenated index table) built alone, packed tight in list order."""
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    built = [L.build(vertices, indices[f: f + n], max_leaf) for f, n in np.asarray(ranges)]
    nodes, tris, table = M.pack([b[:2] for b in built])
    return nodes, tris, table, np.array([b[2] for b in built], np.int32)


def objects_of(nodes, tris, table):
    """[(nodes, tris)] per object of a packed set."""
    return [(nodes[r["node_offset"]: r["node_offset"] + r["num_nodes"]], tris[r["tri_offset"]: r["tri_offset"] + r["num_tris"]])
            for r in table]


def slots(ranges):
    """(node_offset, capacity) per object of a slotted set: a slot of max(1, n - 1) records each, one behind the other."""
    room = np.maximum(np.asarray(ranges)[:, 1].astype(np.int64) - 1, 1)
    return np.cumsum(room) - room, room


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def concat(meshes):
    """(vertices (nv, 4), indices (n, 4), ranges (K, 2)) of [(vertices, indices)] meshes with object-local vertex ids."""
    vertices, indices, ranges, base, row = [], [], [], 0, 0
    for v, ix in meshes:
        v = np.asarray(v, F32).reshape(len(v), -1)
        v4 = np.zeros((len(v), 4), F32); v4[:, : v.shape[1]] = v
        ix = np.asarray(ix, np.int32).reshape(len(ix), -1)
        i4 = np.zeros((len(ix), 4), np.int32); i4[:, : ix.shape[1]] = ix
        i4[:, :3] += base
        ranges.append((row, len(i4)))
        vertices.append(v4); indices.append(i4)
        base += len(v4); row += len(i4)
    return np.concatenate(vertices), np.concatenate(indices), np.int32(ranges)


def seeded(n, seed, extent=10.0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-extent, extent, (n, 1, 3))
    v = (centre + rng.normal(0, 0.3, (n, 3, 3))).astype(F32).reshape(3 * n, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


SINGLE, PAIR, FLAT, SOUP67, EQUAL40, FLAT_AXIS, BIG, SOUP_SCALED = range(8)


def fixture_meshes():
    """The eight objects, in list order: one triangle; two triangles; the flat quad (z constant); a 67-triangle indexed soup; 40
    identical triangles (every code equal; its first sorted position, 72, is no multiple of 64, so global and local tie-breaks differ);
    53 triangles flat on x (scale 0); 5 000 seeded triangles (from position 165 on: across a 4 096-key radix tile and many 256-thread
    blocks, starting mid-tile); the soup again scaled by 2^10 (a frame shared with any other object would change its codes)."""
    z = 0.5
    soup_v, soup_ix = SU.indexed_soup(67, 68)[:2]
    one = F32([[0.25, 0.5, -1.0], [1.25, 0.5, -0.5], [0.25, 1.5, 0.0]])
    flat_v, flat_ix = seeded(53, 7)
    flat_v[:, 0] = 3.0
    meshes = [(F32([[0, 0, 0], [1, 0, 0.5], [0, 1, 1]]), [[0, 1, 2]]),
              (F32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 7]]), [[0, 1, 2], [3, 4, 5]]),
              (F32([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]]), [[0, 1, 2], [0, 2, 3]]),
              (soup_v, soup_ix),
              (one, np.tile(np.int32([[0, 1, 2]]), (40, 1))),
              (flat_v, flat_ix),
              seeded(5000, 11),
              (np.asarray(soup_v, F32) * F32(1024), soup_ix)]
    assert sum(len(ix) for _, ix in meshes[:EQUAL40]) % 64 != 0
    return meshes


def many_meshes(count=300, seed=3):
    """`count` objects of one to three triangles: more than 256 listed objects, so the rank takes a second radix digit."""
    rng = np.random.default_rng(seed)
    return [seeded(int(rng.integers(1, 4)), 1000 + k, extent=float(rng.uniform(0.5, 50))) for k in range(count)]


# ---- perturbed models -----------------------------------------------------------------------------------------------------------------
class _patched:
    def __init__(self, **names):
        self.names, self.saved = names, {}

    def __enter__(self):
        for k, v in self.names.items():
            self.saved[k] = getattr(L, k); setattr(L, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(L, k, v)


def _delta_with_offset(offset):
    """lbvh_model._delta with the tie rule on positions moved by `offset`: 32 + clz((i + offset) ^ (j + offset))."""
    def delta(codes, i, j):
        n = len(codes)
        inside = (j >= 0) & (j < n)
        jj = np.where(inside, j, 0)
        x = codes[i] ^ codes[jj]
        gi, gj = i + offset, jj + offset
        out = np.where(x != 0, L._clz32(np.where(x != 0, x, 1)), 32 + L._clz32(np.where(gi != gj, gi ^ gj, 1)))
        return np.where(inside, out, -1)
    return delta


def build_global_ties(vertices, indices, ranges, max_leaf=2):
    """The model with equal codes told apart by GLOBAL sorted positions (the object's first position added to both)."""
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    built, start = [], 0
    for f, n in np.asarray(ranges):
        with _patched(_delta=_delta_with_offset(start)):
            built.append(L.build(vertices, indices[f: f + n], max_leaf))
        start += n
    return (*M.pack([b[:2] for b in built]), np.array([b[2] for b in built], np.int32))


def build_shared_frame(vertices, indices, ranges, max_leaf=2):
    """The model with ONE frame for all listed objects: codes over the bounds of all their centroid sums."""
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    rows = np.concatenate([np.arange(f, f + n) for f, n in np.asarray(ranges)])
    v = L.load_triangles(vertices, indices[rows])[0]
    codes, built, start = L.morton_codes(L.triangle_references(v)[2]), [], 0
    for f, n in np.asarray(ranges):
        with _patched(morton_codes=lambda points, c=codes[start: start + n]: c):
            built.append(L.build(vertices, indices[f: f + n], max_leaf))
        start += n
    return (*M.pack([b[:2] for b in built]), np.array([b[2] for b in built], np.int32))


def karras_unbounded(vertices, indices, ranges):
    """Per object (first, last, split) of a Karras search over the objects' sorted codes laid end to end that is bounded by the TOTAL
    only: j beyond the object reads the neighbour's codes (ties by local positions, as the true rule).  Ranges may leave the object,
    so no tree can be emitted from them; at max_leaf 1 every node is kept and the tree's child words state (first, last, split), so
    arrays that differ from lbvh_model.karras' are bytes that differ."""
    indices = np.asarray(indices, np.int32).reshape(-1, 4)
    sorted_codes = []
    for f, n in np.asarray(ranges):
        v, geom, _ = L.load_triangles(vertices, indices[f: f + n])
        sorted_codes.append(L.sort_references(v, geom, *L.triangle_references(v))[0])
    every = np.concatenate(sorted_codes)
    out, start = [], 0
    for codes in sorted_codes:
        n = len(codes)
        if n < 2:
            out.append(None); start += n
            continue

        def delta(_, i, j, start=start):
            gi, gj = i + start, j + start
            inside = (gj >= 0) & (gj < len(every))
            jj = np.where(inside, gj, 0)
            x = every[gi] ^ every[jj]
            ties = 32 + L._clz32(np.maximum((i ^ j) & 0x7FFFFFFF, 1))
            return np.where(inside, np.where(x != 0, L._clz32(np.where(x != 0, x, 1)), ties), -1)
        with _patched(_delta=delta):
            out.append(L.karras(codes))
        start += n
    return out, [None if len(c) < 2 else L.karras(c) for c in sorted_codes]
