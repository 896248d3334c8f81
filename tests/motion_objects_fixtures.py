"""The scene, times and rays that tests/test_motion_objects_model.py (CPU) and tests/test_gpu_motion_objects.py share, and the conditions
they must meet so that no GPU test passes vacuously (check_conditions; the CPU test runs them on the model alone).

Objects, each with two keys over one concatenated vertex / index table:
  0 SHEARED   the cube of motion_instance_fixtures (12 triangles), key 1 sheared and lifted
  1 CUBE      the same cube with key 1 equal to key 0
  2 SOUP      200 seeded triangles in [-0.5, 0.5]^3, key 1 by motion_bvh_fixtures.displace
  3 SINGLE    one triangle: a one-leaf root beside an empty slot; key 1 turned in its plane and pushed along z
  4 BOX       the Cornell box (the triangles of tests/golden/cornell.bvh's BVH2 block, one row per record) with equal keys
Every topology is lbvh_model.build(max_leaf 2) of key 0.  Nine instances at motion_instance_fixtures.layout()'s placements: its boxes
stay the Cornell box, its cubes become the objects above -- the half turn (singular at t = 0.5) places CUBE, the mirrored cube places
SOUP, the wall behind everything is SOUP flattened, SINGLE stands in front.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import lbvh_model as L
import motion_bvh_fixtures as BX
import motion_bvh_model as B
import motion_instance_fixtures as IX
import motion_instance_model as MI
import motion_objects_model as MO
from rodent_amd import formats as F

F32 = np.float32
SHEARED, CUBE, SOUP, SINGLE, BOX = range(5)
# layout()'s nine placements, in its order: which object each places
OBJECT_OF = np.array([BOX, SHEARED, SOUP, CUBE, BOX, SINGLE, SHEARED, BOX, SOUP], np.int32)
HALF_TURN = IX.HALF_TURN
EXTRA_TIMES = np.array([-0.0, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1)), np.inf, -np.inf,
                        np.nextafter(F32(1), F32(2)), -(2.0 ** -149)], F32)


def palette():
    """motion_instance_fixtures' 16 times (0, 1, 0.5, NaN, times outside [0, 1] and seeded ones among them) and the 7 above: 23 values,
    no two with the same bits."""
    p = np.concatenate([IX.palette(), EXTRA_TIMES])
    assert len(set(p.view("<u4").tolist())) == len(p) == 23
    return p


def times_for(n):
    """The palette cycled over n rays: every wave holds refused times beside traced ones."""
    return palette()[np.arange(n) % 23]


def cube_mesh():
    c = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    v = np.zeros((8, 4), F32); v[:, :3] = c
    ix = np.zeros((12, 4), np.int32)
    for k, (a, b, c_, d) in enumerate(quads):
        ix[2 * k, :3], ix[2 * k + 1, :3] = (a, b, c_), (a, c_, d)
    return v, ix


def soup_mesh(n=200, seed=57):
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), F32)
    centre = rng.uniform(-0.4, 0.4, (n, 1, 3))
    v[:, :3] = np.clip(centre + rng.uniform(-0.16, 0.16, (n, 3, 3)), -0.5, 0.5).reshape(-1, 3).astype(F32)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


def box_mesh(block):
    """The triangles of a BVH2 / Tri1 block as a mesh: three vertices of its own per record, row k = record k."""
    tris = block[1]
    v = np.zeros((3 * len(tris), 4), F32)
    v0 = tris["v0"].astype(F32)
    v[0::3, :3], v[1::3, :3], v[2::3, :3] = v0, v0 - tris["e1"], v0 + tris["e2"]
    ix = np.zeros((len(tris), 4), np.int32)
    ix[:, :3] = np.arange(3 * len(tris)).reshape(-1, 3)
    return v, ix


def meshes(block):
    """[(key 0 vertices, key 1 vertices, index rows)] of the five objects, each with vertex ids of its own."""
    cv, cix = cube_mesh()
    sheared = cv.copy()
    sheared[:, 0] += F32(0.7) * cv[:, 1]; sheared[:, 1] += F32(0.25); sheared[:, 2] *= F32(0.6)
    sv, six = soup_mesh()
    single = np.zeros((3, 4), F32); single[:, :3] = [[-0.5, -0.5, 0.1], [0.5, -0.5, 0.1], [0.0, 0.5, 0.1]]
    single1 = np.zeros((3, 4), F32); single1[:, :3] = [[-0.5, 0.3, -0.3], [0.3, -0.5, -0.3], [0.5, 0.5, -0.3]]
    bv, bix = box_mesh(block)
    one = np.zeros((1, 4), np.int32); one[0, :3] = (0, 1, 2)
    return [(cv, sheared, cix), (cv, cv.copy(), cix), (sv, BX.displace(sv, 91, 0.2), six), (single, single1, one), (bv, bv.copy(), bix)]


def concatenate(parts):
    """(vertices0, vertices1, indices, ranges) of the concatenated tables: vertex ids offset, one (first_tri, num_tris) row per object."""
    v0, v1, ix, ranges, nv, nt = [], [], [], [], 0, 0
    for a, b, rows in parts:
        rows = rows.copy(); rows[:, :3] += nv
        v0.append(a); v1.append(b); ix.append(rows); ranges.append((nt, len(rows)))
        nv += len(a); nt += len(rows)
    return np.concatenate(v0), np.concatenate(v1), np.concatenate(ix), np.array(ranges, np.int32)


class Scene:
    """The model's side: the concatenated meshes, the packed topologies, the motion records, the descriptors and the motion TLAS.
    freeze_objects: key 1 = key 0 everywhere; freeze_placements: M1 = M0 everywhere (what the conditions compare with)."""

    def __init__(self, block, max_leaf=1, freeze_objects=False, freeze_placements=False, topology_leaf=2):
        self.v0, self.v1, self.ix, self.ranges = concatenate(meshes(block))
        if freeze_objects:
            self.v1 = self.v0.copy()
        self.pairs = []
        for first, count in self.ranges:
            nodes, tris, info = L.build(self.v0, self.ix[first: first + count], topology_leaf)
            assert info[2] == 0
            self.pairs.append((nodes, tris))
        self.nodes, self.tris, self.table = M.pack(self.pairs)
        self.mn, self.mt, self.build_info = MO.build(self.nodes, self.tris, self.table, self.v0, self.v1, self.ix, self.ranges)
        assert self.build_info.tolist() == [len(self.nodes), len(self.nodes) + len(self.tris), 0, len(self.nodes)]
        self.t0, self.t1, _, self.ids = IX.layout()
        if freeze_placements:
            self.t1 = self.t0.copy()
        self.obj = OBJECT_OF
        self.descs = MI.descriptors(self.t0, self.t1, self.obj, self.ids)
        self.tlas, self.inst, self.info = MO.build_motion_tlas(self.mn, self.table, self.descs, max_leaf)
        assert self.info[2] == 0

    def model(self):
        return self.tlas, self.inst, self.mn, self.mt


def ray_sets(cornell):
    """{name: rays}: the three Cornell ray sets of tests/golden and 4096 seeded segments through the room."""
    sets = {name: cornell.ray_sets[name] for name in ("primary", "random", "edge")}
    sets["segments"] = BX.segments(np.array([-1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.2]), 4096, 77)
    return sets


def check_conditions(oracle, block, cornell):
    """The conditions on the model alone; returns the figures for the caller to print."""
    full, still, parked = Scene(block), Scene(block, freeze_objects=True), Scene(block, freeze_placements=True)
    single_ids = set(int(i) for i in full.ids[OBJECT_OF == SINGLE])
    out, both, seen = {}, 0, set()
    for name, rays in ray_sets(cornell).items():
        times = times_for(len(rays))
        on = B.traced(times)
        h, i = MO.trace(oracle, *full.model(), rays, times)
        hs, is_ = MO.trace(oracle, *still.model(), rays, times)
        hp, ip = MO.trace(oracle, *parked.model(), rays, times)
        assert (h["tri_id"][~on] == -1).all() and (i[~on] == -1).all()
        hit = h["tri_id"] >= 0
        share = float(hit[on].mean())
        assert share >= 0.25, (name, share)
        differs = lambda a, b: (a["tri_id"] != h["tri_id"]) | (a["t"] != h["t"]) | (b != i)
        d_objects, d_placements = float(differs(hs, is_)[hit].mean()), float(differs(hp, ip)[hit].mean())
        assert d_objects >= 0.10 and d_placements >= 0.10, (name, d_objects, d_placements)
        both += int((hit & (hs["tri_id"] < 0) & (hp["tri_id"] < 0)).sum())
        seen |= set(int(k) for k in i[hit])
        out[name] = (share, d_objects, d_placements)
    assert both >= 1                                                     # a ray that hits only when both motions are on
    assert len(seen) >= 4 and seen & single_ids, seen
    out["both"], out["instances"] = both, sorted(seen)
    return out
