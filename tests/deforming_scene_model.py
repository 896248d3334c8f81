"""CPU model of deforming meshes in the renderer (include/rodent_render.h, "deforming meshes in the renderer"; csrc/render_deforming.h,
k_shade<.., false, DeformingDev>) in numpy, over motion_bvh_model (the motion records and their traversal with a time per ray),
scene_update_model (the face-normal and smooth-normal rules), motion_scene_model (the third draw, the shutter rule, the depth word) and
oracle.binding (the flat shader), all four as they stand.

  keys, records   the tables rodent_hip_scene_create_deforming / _set_motion_keys hold: both keys' vertices and normals, the records
  moving_light    the creation's refusal: an emissive triangle whose corner rows differ in a byte between the keys
  lerp_rows       rows at a time per row: s = 1 - t; s * x0 + t * x1, every operation rounded to float32
  bake_hits       a flat scene of ONE triangle per hit: corners and corner normals interpolated to the hit's time, the face normal by
                  the moved-geometry rule on those corners, plus the static lights (key 0's: the TRAVERSAL reaches an emitter through
                  s * x + t * x, which equals x only up to the rounding of that sum; its light record is x): flat shading of it is,
                  bit for bit, the deforming shading
  frame           motion_scene_model.frame's shape with motion_bvh_model.trace
numpy float32 arithmetic is correctly rounded operation by operation, like the kernels under -ffp-contract=off.
"""
from __future__ import annotations

import numpy as np

import motion_bvh_model as MB
import motion_scene_model as MS
import scene_update_model as SU
from oracle import binding as O
from rodent_amd import formats as F
from shade_fixtures import FLT_MAX_REF, RAY_OFFSET, SHADOW_TMAX

F32 = np.float32
DEPTH_BITS, DEPTH_MASK = MS.DEPTH_BITS, MS.DEPTH_MASK
third_draw, shutter_time, pack = MS.third_draw, MS.shutter_time, MS.pack


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
class Keys:
    """vertices0, vertices1, normals0, normals1: (num_vertices, 4) float32, the mesh at time 0 and at time 1."""

    def __init__(self, vertices0, vertices1, normals0, normals1):
        self.vertices0, self.vertices1, self.normals0, self.normals1 = (np.ascontiguousarray(a, F32).reshape(-1, 4) for a in
                                                                        (vertices0, vertices1, normals0, normals1))


def smooth_keys(vertices0, vertices1, indices):
    """The keys as rodent_hip_scene_set_motion_keys leaves them when no normals are given: per key the face normals of that key, summed
    over each vertex's incidence list (scene_update_model)."""
    nv = len(vertices0)
    n0, n1 = (SU.smooth_normals(SU.face_normals(v, indices), indices, nv) for v in (vertices0, vertices1))
    return Keys(vertices0, vertices1, n0, n1)


def records(topology, keys, indices):
    """(motion nodes, motion tris, info) of rodent_hip_build_motion_bvh2_tri1 over the static key-0 topology (nodes, tris)."""
    return MB.build(topology[0], topology[1], keys.vertices0, keys.vertices1, indices)


def moving_light(scene, vertices1):
    """Whether rodent_hip_scene_create_deforming refuses key 1: an emissive triangle one of whose three corner rows (16 bytes) differs
    in a byte from key 0's."""
    v0, v1 = np.ascontiguousarray(scene.vertices, F32).reshape(-1, 4), np.ascontiguousarray(vertices1, F32).reshape(-1, 4)
    ix = np.asarray(scene.indices).reshape(-1, 4)
    emissive = np.asarray(scene.materials)["emissive"][ix[:, 3]] != 0
    rows = np.unique(ix[emissive, :3])
    return bool((v0[rows].view("<u4") != v1[rows].view("<u4")).any())


# ---- hits, baked at their own times -------------------------------------------------------------------------------------------------------
def lerp_rows(x0, x1, times):
    """Row q of x0 / x1 at times[q]."""
    t = np.asarray(times, F32)[:, None]
    with np.errstate(all="ignore"):
        s = F32(1) - t
        return (s * np.asarray(x0, F32) + t * np.asarray(x1, F32)).astype(F32)


def face_normals_of(corners):
    """(n, 3) face normals of the (n, 3 corners, 3) triangles by the moved-geometry rule: c = (v1 - v0) x (v2 - v0),
    c * (1 / sqrt((c.x c.x + c.y c.y) + c.z c.z))."""
    with np.errstate(all="ignore"):
        a, b = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)
        return (c * (F32(1.0) / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]))[:, None]).astype(F32)


class Baked:
    @property
    def num_tris(self):
        return len(self.indices)


def bake_hits(scene, keys, lights, prims, times, face_rule="corners"):
    """The flat scene of one triangle per hit: triangle q is triangle prims[q] at times[q], with three fresh vertices 3q, 3q + 1, 3q + 2.
    face_rule "corners" is the renderer's; "lerp" -- the normalised interpolation of the two keys' face normals -- is the WRONG rule the
    fixtures show to be detectable."""
    prims, times = np.asarray(prims, np.int64), np.asarray(times, F32)
    ind = np.asarray(scene.indices)[prims]
    corners = ind[:, :3].reshape(-1)
    vt = np.repeat(times, 3)
    out = Baked()
    out.vertices = np.array(keys.vertices0[corners])                              # (the fourth word: key 0's)
    out.vertices[:, :3] = lerp_rows(keys.vertices0[corners, :3], keys.vertices1[corners, :3], vt)
    out.normals = np.array(keys.normals0[corners])
    out.normals[:, :3] = lerp_rows(keys.normals0[corners, :3], keys.normals1[corners, :3], vt)
    out.face_normals = np.zeros((len(prims), 4), F32)
    if face_rule == "corners":
        out.face_normals[:, :3] = face_normals_of(out.vertices[:, :3].reshape(-1, 3, 3))
    else:
        f0, f1 = (face_normals_of(k[corners, :3].reshape(-1, 3, 3)) for k in (keys.vertices0, keys.vertices1))
        f = lerp_rows(f0, f1, times)
        with np.errstate(all="ignore"):
            out.face_normals[:, :3] = f * (F32(1.0) / np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]))[:, None]
    out.texcoords = np.array(np.asarray(scene.texcoords, F32)[corners])
    q = np.arange(len(prims), dtype=np.int32)
    out.indices = np.stack([3 * q, 3 * q + 1, 3 * q + 2, ind[:, 3]], 1).astype(np.int32)
    out.light_ids = np.asarray(scene.light_ids)[prims].astype(np.int32)
    out.lights = lights
    out.materials, out.textures, out.texels = scene.materials, scene.textures, scene.texels
    out.nodes, out.tris = np.zeros(0, F.NODE2), np.zeros(0, F.TRI1)
    return out


# ---- a frame ----------------------------------------------------------------------------------------------------------------------------
class Frame:
    """film (h, w, 3) float32, counts [primary rays, shadow rays], and per bounce what was traced: `primary` (rays RAY1, pixel ids, hits
    HIT1, ubits), `shadow` (rays, pixel ids, hits, colours, times) and `vertices` (ORACLE_VERTEX records with prim = the hit's index
    in that bounce's bake, pixel ids, the scene's prim ids, ubits); `rnd` and `ubits` are the camera rays' state behind the third draw
    and their time bits; `nodes` / `tris` the motion records."""


def frame(scene, keys, topology, cam, iter_, spp, max_path_len, width, height, shutter=(0.0, 1.0)):
    """One frame of the deforming scene: motion_scene_model.frame over one mesh.  Per pixel the additions happen in oracle_render's
    order, in float32."""
    mn, mt, info = records(topology, keys, scene.indices)
    assert info[2] == 0 and info[0] == info[3] == len(topology[0]) and not moving_light(scene, keys.vertices1)
    lights = scene.lights
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
    out.nodes, out.tris, out.lights, out.rnd, out.ubits = mn, mt, lights, rnd, ubits
    while len(v):
        rays = F.make_rays(v["org"], v["dir"], tmin, FLT_MAX_REF)
        times = shutter_time(ubits[path], *shutter)
        hits = MB.trace(O, mn, mt, rays, times)
        out.primary.append((rays, path // spp, hits, ubits[path])); out.counts[0] += len(rays)
        hit = hits["tri_id"] >= 0
        v, path, hits, times = v[hit], path[hit], hits[hit], times[hit]
        if not len(v):
            break
        flat = bake_hits(scene, keys, lights, hits["tri_id"], times)
        v["prim"] = np.arange(len(v)); v["t"] = hits["t"]; v["u"] = hits["u"]; v["v"] = hits["v"]
        out.vertices.append((v.copy(), path // spp, hits["tri_id"].copy(), ubits[path]))
        o = O.shade_vertices(flat, v, max_path_len)
        sh = o["shadow"] != 0
        srays = F.make_rays(o["s_org"][sh], o["s_dir"][sh], RAY_OFFSET, SHADOW_TMAX)
        occl = MB.trace(O, mn, mt, srays, times[sh], any_hit=True)
        out.shadow.append((srays, path[sh] // spp, occl, o["s_color"][sh], times[sh])); out.counts[1] += len(srays)
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
