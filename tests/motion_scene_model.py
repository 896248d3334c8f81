"""CPU model of moving instances in the renderer (include/rodent_render.h, "moving instances in the renderer"; csrc/render_motion.h) in
numpy, over motion_instance_model (the motion TLAS and its traversal with a time per ray), instanced_scene_model (the derived tables,
the corner and normal rules) and oracle.binding (the flat shader), all three as they stand.

  third_draw, shutter_time   the path's shutter sample (the third randf behind the pixel sample's two) and the shutter rule in float32
  tlas_of, world_lights      the tables rodent_hip_scene_create_motion derives (slot_of, bases, light_owner: instanced_scene_model's)
  bake_hits                  a flat scene of ONE triangle per hit, placed by lerp(M0, M1, t) of the hit's own time and its inverse, plus
                             the static world lights: flat shading of it is, bit for bit, the moving shading
  frame                      instanced_scene_model.frame's shape with motion_instance_model.trace and a time per path
  placements, crafted_rays   the test scene and the crafted trace set
numpy float32 arithmetic is correctly rounded operation by operation, like the kernels under -ffp-contract=off.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import instanced_scene_model as IM
import motion_instance_model as MM
from oracle import binding as O
from rodent_amd import formats as F
from shade_fixtures import FLT_MAX_REF, RAY_OFFSET, SHADOW_TMAX

F32 = np.float32
DEPTH_BITS, DEPTH_MASK = 8, 0xFF                      # RODENT_MOTION_DEPTH_BITS, RODENT_MOTION_DEPTH_MASK
W, H, SPP, MAXLEN = 32, 24, 2, 4


# ---- the time of a path -----------------------------------------------------------------------------------------------------------------
def xorshift(state):
    """random.impala:22-30 over uint32 arrays: the next state (which is also the draw)."""
    x = np.asarray(state, np.uint32).copy()
    x[x == 0] = 1
    x ^= x << np.uint32(13); x ^= x >> np.uint32(17); x ^= x << np.uint32(5)
    return x


def third_draw(rnd):
    """(the random state behind the draw, ubits): u = randf(&rnd) = ubits * 2^-23 with ubits the draw's low 23 bits."""
    x = xorshift(rnd)
    return x, (x & np.uint32(0x7FFFFF)).astype(np.int32)


def shutter_time(ubits, open_, close):
    """t = min(close, open + (close - open) * u), u = ubits * 2^-23: difference, product and sum each rounded to float32."""
    u = np.asarray(ubits).astype(F32) * F32(2.0 ** -23)                   # exact: ubits < 2^24
    o, c = F32(open_), F32(close)
    return np.minimum(c, (o + ((c - o) * u).astype(F32)).astype(F32)).astype(F32)


def pack(depth, ubits):
    return (np.asarray(depth, np.int64) | np.asarray(ubits, np.int64) << DEPTH_BITS).astype(np.int32)


# ---- the derived tables -----------------------------------------------------------------------------------------------------------------
def tlas_of(nodes, table, transforms0, transforms1, object_ids):
    """(tlas nodes, MOTION_INSTANCE records in leaf order, info) as the scene builds them: ids 0 ... n - 1, max_leaf 1."""
    return MM.build_motion_tlas(nodes, table, MM.descriptors(transforms0, transforms1, object_ids), 1)


def world_lights(object_lights, ranges, transforms0, object_ids):
    """The static world lights: instanced_scene_model's under M0 (an emitter has M0 == M1)."""
    return IM.world_lights(object_lights, ranges, transforms0, object_ids)


def moving_light(ranges, transforms0, transforms1, object_ids):
    """Whether rodent_hip_scene_create_motion refuses the placements: an instance of an object with lights whose keys differ in a byte."""
    t0 = np.ascontiguousarray(transforms0, F32).reshape(-1, 12); t1 = np.ascontiguousarray(transforms1, F32).reshape(-1, 12)
    lit = np.asarray(ranges)[np.asarray(object_ids), 3] > 0
    return bool(any(t0[k].tobytes() != t1[k].tobytes() for k in np.flatnonzero(lit)))


# ---- hits, baked at their own times -------------------------------------------------------------------------------------------------------
def bake_hits(scene, ranges, transforms0, transforms1, object_ids, lights, inst, local, times):
    """The flat scene (instanced_scene_model.Baked) of one triangle per hit: triangle q is triangle local[q] of instance inst[q]'s
    object under m = lerp(M0, M1, times[q]) and w = invert(m), by instanced_scene_model.baked's rules; `lights` are the static world
    lights.  A hit lies in an instance that was not skipped, so the inverse exists."""
    ranges, object_ids = np.asarray(ranges, np.int64), np.asarray(object_ids)
    inst, local = np.asarray(inst, np.int64), np.asarray(local, np.int64)
    t0 = np.asarray(transforms0, F32).reshape(-1, 12); t1 = np.asarray(transforms1, F32).reshape(-1, 12)
    m = MM.lerp(t0[inst], t1[inst], np.asarray(times, F32))
    w, refused = M.invert(m)
    assert not refused.any()
    b = IM.bases(ranges, object_ids)
    gprim = ranges[object_ids[inst], 0] + local
    ind = np.asarray(scene.indices)[gprim]
    corners = ind[:, :3].reshape(-1)
    vq = np.repeat(np.arange(len(inst)), 3)
    out = IM.Baked()
    out.vertices = np.array(np.asarray(scene.vertices, F32)[corners])
    out.vertices[:, :3] = IM.map_points(m[vq], out.vertices[:, :3])
    out.normals = np.array(np.asarray(scene.normals, F32)[corners])
    out.normals[:, :3] = IM.map_normals(w[vq], out.normals[:, :3])
    out.face_normals = np.array(np.asarray(scene.face_normals, F32)[gprim])
    out.face_normals[:, :3] = IM.normalized(IM.map_normals(w, out.face_normals[:, :3]))
    out.texcoords = np.array(np.asarray(scene.texcoords, F32)[corners])
    q = np.arange(len(inst), dtype=np.int32)
    out.indices = np.stack([3 * q, 3 * q + 1, 3 * q + 2, ind[:, 3]], 1).astype(np.int32)
    emissive = np.asarray(scene.materials)["emissive"][ind[:, 3]] != 0
    out.light_ids = np.where(emissive, np.asarray(scene.light_ids)[gprim] + b[inst, 1], 0).astype(np.int32)
    out.lights = lights
    out.materials, out.textures, out.texels = scene.materials, scene.textures, scene.texels
    out.nodes, out.tris = np.zeros(0, F.NODE2), np.zeros(0, F.TRI1)
    return out


# ---- a frame ----------------------------------------------------------------------------------------------------------------------------
class Frame:
    """film (h, w, 3) float32, counts [primary rays, shadow rays], and per bounce what was traced: `primary` (rays RAY1, pixel ids, hits
    HIT1, instance ids, ubits), `shadow` (rays, pixel ids, hits, instance ids, colours, times) and `vertices` (ORACLE_VERTEX records
    with prim = the hit's index in that bounce's bake, pixel ids, instance ids, object-local prim ids, ubits); `rnd` and `ubits` are
    the camera rays' state behind the third draw and their time bits."""


def frame(scene, ranges, transforms0, transforms1, object_ids, hierarchy, cam, iter_, spp, max_path_len, width, height,
          shutter=(0.0, 1.0)):
    """One frame of the moving scene: instanced_scene_model.frame with a time per path.  Per pixel the additions happen in
    oracle_render's order, in float32."""
    nodes, tris, table = hierarchy
    tlas, minst, info = tlas_of(nodes, table, transforms0, transforms1, object_ids)
    assert info[2] == 0 and not moving_light(ranges, transforms0, transforms1, object_ids)
    lights = world_lights(scene.lights, ranges, transforms0, object_ids)
    max_path_len = min(max_path_len, DEPTH_MASK)
    y, x, sample = [a.reshape(-1) for a in np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")]
    rnd, d = O.emit_samples(cam, iter_, width, height, x, y, sample)
    rnd, ubits = third_draw(rnd)
    n = len(rnd)
    v = np.zeros(n, O.ORACLE_VERTEX)
    v["org"] = np.asarray(cam["eye"], "<f4"); v["dir"] = d; v["rnd"] = rnd; v["contrib"] = 1.0
    path = np.arange(n)
    tmin = np.zeros(n, "<f4")
    inv_spp = F32(1.0) / F32(spp)
    adds = [[] for _ in range(n)]
    out = Frame()
    out.primary, out.shadow, out.vertices, out.counts = [], [], [], [0, 0]
    out.tlas, out.instances, out.lights, out.rnd, out.ubits = tlas, minst, lights, rnd, ubits
    while len(v):
        rays = F.make_rays(v["org"], v["dir"], tmin, FLT_MAX_REF)
        times = shutter_time(ubits[path], *shutter)
        hits, ids = MM.trace(O, tlas, minst, nodes, tris, rays, times)
        out.primary.append((rays, path // spp, hits, ids, ubits[path])); out.counts[0] += len(rays)
        hit = hits["tri_id"] >= 0
        v, path, hits, ids, times = v[hit], path[hit], hits[hit], ids[hit], times[hit]
        if not len(v):
            break
        flat = bake_hits(scene, ranges, transforms0, transforms1, object_ids, lights, ids, hits["tri_id"], times)
        v["prim"] = np.arange(len(v)); v["t"] = hits["t"]; v["u"] = hits["u"]; v["v"] = hits["v"]
        out.vertices.append((v.copy(), path // spp, ids, hits["tri_id"].copy(), ubits[path]))
        o = O.shade_vertices(flat, v, max_path_len)
        sh = o["shadow"] != 0
        srays = F.make_rays(o["s_org"][sh], o["s_dir"][sh], RAY_OFFSET, SHADOW_TMAX)
        occl, oids = MM.trace(O, tlas, minst, nodes, tris, srays, times[sh], any_hit=True)
        out.shadow.append((srays, path[sh] // spp, occl, oids, o["s_color"][sh], times[sh])); out.counts[1] += len(srays)
        lit = np.zeros(len(v), bool); lit[np.flatnonzero(sh)[occl["tri_id"] < 0]] = True
        for k in np.flatnonzero(o["emits"] != 0):
            adds[path[k]].append(o["emitted"][k] * inv_spp)
        for k in np.flatnonzero(lit):
            adds[path[k]].append(o["s_color"][k] * inv_spp)
        b = o["bounce"] != 0
        nv = np.zeros(int(b.sum()), O.ORACLE_VERTEX)
        nv["org"] = o["b_org"][b]; nv["dir"] = o["b_dir"][b]; nv["rnd"] = o["rnd"][b]; nv["mis"] = o["mis"][b]
        nv["contrib"] = o["contrib"][b]; nv["depth"] = v["depth"][b] + 1
        v, path = nv, path[b]
        tmin = np.full(len(v), RAY_OFFSET, "<f4")
    film = np.zeros((height * width, 3), "<f4")
    for k, a in enumerate(adds):
        for term in a:
            film[k // spp] += term
    out.film = film.reshape(height, width, 3)
    return out


# ---- the test scene ---------------------------------------------------------------------------------------------------------------------
BOX, QUAD_A, QUAD_B, SLIDER, TUMBLER, MIRRORED, HALF_TURN = range(7)
MOVERS = (SLIDER, TUMBLER, MIRRORED, HALF_TURN)


def placements():
    """(transforms0, transforms1 (7, 12) float32, object ids) over instanced_scene_model.scene_objects: the box, static; both emissive
    quads, static with M0 == M1 byte for byte (one under a mirroring matrix); a cube translating by its own width; a cube with an
    oblique rotation plus a non-uniform scale between its keys; a mirrored cube, moving; a cube on a half turn about y, whose
    interpolated matrix is diag(0, s, 0) at t = 0.5 exactly (ubits = 2^22)."""
    def place(linear, translation):
        t = np.zeros((3, 4)); t[:, :3] = linear; t[:, 3] = translation
        return t
    R = IM._rotation
    t0 = [place(np.eye(3), (0, 0, 0)),
          place(R((0, 1, 0), 0.3) @ np.diag([0.5, 1.0, 0.5]), (-0.5, 1.6, 0.2)),
          place(R((0, 0, 1), 0.15) @ np.diag([-0.25, 1.0, 0.35]), (0.55, 1.4, -0.3)),
          place(np.diag([0.3, 0.3, 0.3]), (-0.7, 0.3, 0.4)),
          place(R((1, 2, 0.5), 0.9) @ np.diag([0.35, 0.5, 0.25]), (0.65, 1.1, -0.3)),
          place(R((0, 1, 0), 0.5) @ np.diag([-0.3, 0.3, 0.3]), (-0.4, 0.2, 0.8)),
          place(np.diag([0.3, 0.3, 0.3]), (0.3, 0.9, 0.3))]
    t1 = [t0[0], t0[1], t0[2],
          place(np.diag([0.3, 0.3, 0.3]), (-0.4, 0.3, 0.4)),
          place(R((1, 2, 0.5), 1.4) @ np.diag([0.3, 0.4, 0.35]), (0.55, 1.2, -0.4)),
          place(R((0, 1, 0), 0.5) @ np.diag([-0.3, 0.3, 0.3]), (-0.25, 0.35, 0.75)),
          None]
    t0 = np.asarray(t0).reshape(7, 12).astype(F32)
    half = t0[HALF_TURN].reshape(3, 4).copy(); half[:, 0] = -half[:, 0]; half[:, 2] = -half[:, 2]      # M0 times diag(-1, 1, -1): exact
    t1[HALF_TURN] = half
    t1 = np.asarray([np.asarray(t, np.float64).reshape(12) for t in t1]).astype(F32)
    t1[:3] = t0[:3]
    return t0, t1, np.array([0, 2, 2, 1, 1, 1, 1], np.int32)


def crafted_rays(transforms0, seed=5):
    """(rays RAY1, ubits): per mover a fan of rays from in front of the scene towards its placement at time 0, each ray four times: at
    ubits 0, 2^22 (t = 0.5 under the shutters (0, 1) and (0.25, 0.75): the half-turn cube is skipped), 2^23 - 1 and a seeded value; and
    rays that leave through the open front."""
    rng = np.random.default_rng(seed)
    t0 = np.asarray(transforms0, np.float64).reshape(-1, 3, 4)
    org, d = [], []
    for k in MOVERS:
        for j in range(6):
            o = np.array([0.25 * np.cos(j + k), 1.0 + 0.04 * j, 2.5])
            org.append(o); d.append(t0[k, :, 3] + 0.05 * np.array([np.sin(3 * j), np.cos(5 * j), 0.0]) - o)
    for j in range(4):
        org.append((0.0, 1.0, 2.7)); d.append((0.3 * j, 5.0 + j, 1.0))
    n = len(org)
    rays = F.make_rays(np.tile(F32(org), (4, 1)), np.tile(F32(d), (4, 1)), 0.0, FLT_MAX_REF)
    ubits = np.concatenate([np.zeros(n), np.full(n, 1 << 22), np.full(n, (1 << 23) - 1), rng.integers(0, 1 << 23, n)]).astype(np.int32)
    return rays, ubits
