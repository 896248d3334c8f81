"""The scene, times and rays that tests/test_motion_instance_model.py (CPU) and tests/test_gpu_motion_instances.py share, and the float64
brute force the model is held to.

Objects: 0 = the Cornell BVH2 block (x in [-1.02, 1], y in [0, 1.99], z in [-1.04, 0.99], open towards +z), 1 = a 12-triangle cube
[-0.5, 0.5]^3 built by lbvh_model.build.  Nine instances, every one of them moving, in the place where the ray sets look for the Cornell box: three reduced copies of
the box (the block holds two of its faces twice, which the brute force cannot tell apart: they are kept small), cubes under mixed
rotations, a non-uniform scale and a mirror, a flattened cube as a wall behind them that leaves part of the view open, and HALF_TURN, a cube whose second placement is its first turned by pi about y -- at t = 0.5 the interpolated matrix is
diag(0, s, 0) exactly, the instance is skipped.  No two instances coincide.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import lbvh_model as L
import motion_instance_model as MM
from rodent_amd import formats as F

F32, F64 = np.float32, np.float64
HALF_TURN = 3                                                           # the instance (and, times 7 plus 2, the instance id) of the half-turn pair
DENORMAL = F32(1e-40)
FIXED_TIMES = np.array([0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24, DENORMAL, np.nan, -0.25, 1.5], F32)


def palette(seed=31):
    """The 16 times of the trace tests: the 9 fixed ones and 7 seeded ones in (0, 1)."""
    return np.concatenate([FIXED_TIMES, np.random.default_rng(seed).uniform(0.0, 1.0, 7).astype(F32)])


def times_for(n, seed):
    return palette()[np.random.default_rng(seed).integers(0, 16, n)]


def cube():
    """(nodes, tris) of the cube [-0.5, 0.5]^3: 12 triangles, max_leaf 2."""
    c = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    v = np.zeros((8, 4), F32); v[:, :3] = c
    ix = np.zeros((12, 4), np.int32)
    for k, (a, b, c_, d) in enumerate(quads):
        ix[2 * k, :3], ix[2 * k + 1, :3] = (a, b, c_), (a, c_, d)
    nodes, tris, info = L.build(v, ix, 2)
    assert info[2] == 0 and len(tris) == 12
    return nodes, tris


def rotation(axis, angle):
    a = np.asarray(axis, F64); a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def place(linear, translation):
    t = np.zeros((3, 4)); t[:, :3] = linear; t[:, 3] = translation
    return t.reshape(12).astype(F32)


def layout():
    """(transforms0, transforms1 (9, 12) float32, object ids, instance ids)."""
    r = rotation
    pairs = [
        (0, place(r((0, 1, 0), 1.6) * 0.5, (-0.75, 0.0, 0.1)), place(r((0, 1, 0), 1.9) * 0.5, (-0.65, 0.1, 0.0))),   # the box, halved
        (1, place(r((1, 2, 0.5), 0.9) @ np.diag([0.5, 0.7, 0.4]), (-0.45, 1.45, 0.3)),
            place(r((1, 2, 0.5), 1.5) @ np.diag([0.5, 0.7, 0.4]), (-0.25, 1.25, 0.1))),
        (1, place(r((0, 1, 0), 0.5) @ np.diag([-0.5, 0.5, 0.5]), (0.6, 0.35, 0.45)),                  # a mirror
            place(r((0, 1, 0), 1.1) @ np.diag([-0.5, 0.5, 0.5]), (0.4, 0.6, 0.25))),
        (1, place(np.eye(3) * 0.4, (0.0, 1.0, 0.2)), place(np.diag([-0.4, 0.4, -0.4]), (0.1, 1.0, 0.2))),   # HALF_TURN
        (0, place(r((0, 0, 1), 0.3) * 0.3, (0.6, 1.1, -0.3)), place(r((0, 0, 1), -0.4) * 0.3, (0.4, 1.3, -0.5))),
        (1, place(r((1, 1, 1), 0.2) * 0.45, (0.55, 1.6, 0.4)), place(r((1, 1, 1), 1.4) * 0.45, (0.45, 1.3, 0.6))),
        (1, place(np.diag([0.9, 0.2, 0.5]), (-0.2, 0.23, 0.6)), place(np.diag([0.5, 0.6, 0.5]), (0.2, 0.3, 0.7))),    # non-uniform
        (0, place(r((0, 1, 0), 2.0) @ np.diag([-0.25, 0.25, 0.25]), (-0.6, 1.0, -0.5)),               # a mirrored small box
            place(r((0, 1, 0), 2.6) @ np.diag([-0.25, 0.25, 0.25]), (-0.7, 0.8, -0.3))),
        (1, place(np.diag([1.6, 1.6, 0.1]), (0.2, 1.0, -0.9)), place(r((0, 1, 0), 0.1) @ np.diag([1.6, 1.6, 0.1]), (0.1, 1.05, -0.8))),
    ]                                                                                                 # (the last: a wall behind them)
    obj = np.array([p[0] for p in pairs], np.int32)
    return np.array([p[1] for p in pairs]), np.array([p[2] for p in pairs]), obj, (np.arange(9) * 7 + 2).astype(np.int64)


class Scene:
    """The model's side: the packed objects, the motion descriptors and the motion TLAS."""

    def __init__(self, block, max_leaf=1):
        self.pairs = [block, cube()]
        self.nodes, self.tris, self.table = M.pack(self.pairs)
        self.t0, self.t1, self.obj, self.ids = layout()
        self.descs = MM.descriptors(self.t0, self.t1, self.obj, self.ids)
        self.tlas, self.inst, self.info = MM.build_motion_tlas(self.nodes, self.table, self.descs, max_leaf)
        assert self.info[2] == 0

    def model(self):
        return self.tlas, self.inst, self.nodes, self.tris

    def num_tris_of(self, slot):
        """The triangle records of the object that the instance in leaf-order slot `slot` places."""
        return int(self.table["num_tris"][np.flatnonzero(self.table["tri_offset"] == self.inst["tri_offset"][slot])[0]])


def ray_sets(cornell):
    """{name: (rays, times)}: the 64 x 64 Cornell primary rays and the 4096 random segments, every ray with a time of the palette."""
    return {name: (cornell.ray_sets[name], times_for(len(cornell.ray_sets[name]), 40 + k)) for k, name in enumerate(("primary", "random"))}


def half_turn_rays(scene, n=256, seed=6):
    """n rays from just in front of the half-turn cube (z = 0.9, clear of the other instances) aimed at points inside its placement at
    time 0."""
    rng = np.random.default_rng(seed)
    m = scene.t0[HALF_TURN].reshape(3, 4).astype(F64)
    target = rng.uniform(-0.4, 0.4, (n, 3)) @ m[:, :3].T + m[:, 3]
    org = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(0.9, 1.1, n), np.full(n, 0.9)], 1)
    return F.make_rays(org.astype(F32), (target - org).astype(F32), 0.0, 100.0)


# ---- the float64 brute force ------------------------------------------------------------------------------------------------------------
GAP = 1e-4           # rays whose nearest two candidates lie closer than this, relative to t, are left out
MARGIN = 1e-5        # a candidate: barycentrics >= -MARGIN and t within GAP (relative) of [tmin, tmax]; the nearest one must lie inside
                     # by the same margins, or the ray is left out too


def brute_force(scene, rays, times):
    """Per ray (instance id, prim id, t, left out) by float64 Moeller-Trumbore over every (instance, triangle) placed at the ray's own
    time: the fp32-interpolated matrix, taken to float64, carries the triangle's corners into the world.  Instances the rule skips are
    left away.  Candidates and the rays left out: GAP and MARGIN above."""
    n = len(rays)
    best_t, second_t = np.full(n, np.inf), np.full(n, np.inf)
    best_inst, best_prim, robust = np.full(n, -1), np.full(n, -1), np.zeros(n, bool)
    org, d = rays["org"].astype(F64), rays["dir"].astype(F64)
    tmin, tmax = rays["tmin"].astype(F64), rays["tmax"].astype(F64)
    inst = scene.inst
    for t, sel in MM.time_groups(times):
        m = MM.lerp(inst["object_to_world0"], inst["object_to_world1"], t)
        _, skipped = M.invert(m)
        for j in np.flatnonzero(~skipped):
            mj = m[j].reshape(3, 4).astype(F64)
            rec = scene.tris[inst["tri_offset"][j]:][: scene.num_tris_of(j)]
            v0, v1, v2 = (rec["v0"].astype(F64), rec["v0"].astype(F64) - rec["e1"], rec["v0"].astype(F64) + rec["e2"])
            v0, v1, v2 = (v @ mj[:, :3].T + mj[:, 3] for v in (v0, v1, v2))
            e1, e2 = (v1 - v0)[None], (v2 - v0)[None]
            o, dd = org[sel][:, None], d[sel][:, None]
            with np.errstate(all="ignore"):
                p = np.cross(dd, e2)
                det = (e1 * p).sum(-1)
                s = o - v0[None]
                u = (s * p).sum(-1) / det
                q = np.cross(s, e1)
                v = (dd * q).sum(-1) / det
                tt = (e2 * q).sum(-1) / det
            lo, hi = tmin[sel][:, None], tmax[sel][:, None]
            inside = (np.minimum(np.minimum(u, v), 1 - u - v) >= -MARGIN) & (tt >= lo - GAP * np.abs(lo)) & (tt <= hi + GAP * np.abs(hi))
            sure = (np.minimum(np.minimum(u, v), 1 - u - v) >= MARGIN) & (tt >= lo + GAP * np.abs(lo)) & (tt <= hi - GAP * np.abs(hi))
            tt = np.where(inside & np.isfinite(tt), tt, np.inf)
            for k in range(tt.shape[1]):
                tk = tt[:, k]
                closer = tk < best_t[sel]
                second_t[sel] = np.where(closer, best_t[sel], np.minimum(second_t[sel], tk))
                best_inst[sel] = np.where(closer, inst["instance_id"][j] & 0x7FFFFFFF, best_inst[sel])
                best_prim[sel] = np.where(closer, rec["prim_id"][k] & 0x7FFFFFFF, best_prim[sel])
                robust[sel] = np.where(closer, sure[:, k], robust[sel])
                best_t[sel] = np.where(closer, tk, best_t[sel])
    hit = np.isfinite(best_t)
    with np.errstate(invalid="ignore"):
        left_out = hit & (~robust | (second_t - best_t <= GAP * np.abs(best_t)))
    return best_inst, best_prim, best_t, left_out
