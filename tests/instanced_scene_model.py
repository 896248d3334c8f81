"""CPU model of instanced scenes in the renderer (include/rodent_render.h, "instanced scenes"; csrc/render_instanced.h) in numpy, over
instance_model (the two-level hierarchy and its traversal) and oracle.binding (the flat shader), both as they stand.

  bases, slot_of, world_lights   the tables rodent_hip_scene_create_instanced derives, byte for byte
  baked                          the instanced scene as a FLAT scene (duck-typed like scene.Scene) whose flat shading is, bit for bit,
                                 the instanced shading: three fresh vertices per (instance, triangle)
  frame                          a CPU path tracer: oracle.emit_samples for the camera rays, instance_model.trace for both passes,
                                 oracle.shade_vertices(baked, ...) for the shader
  scene_objects / placements     the test scene: the Cornell box once, a cube with a mix material four times (oblique rotation with a
                                 non-uniform scale, a mirroring matrix, a pair that coincides exactly), an emissive quad twice
numpy float32 arithmetic is correctly rounded operation by operation, like the kernels under -ffp-contract=off.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import lbvh_model as L
from oracle import binding as O
from rodent_amd import formats as F
from rodent_amd.scene import LIGHT
from shade_fixtures import FLT_MAX_REF, RAY_OFFSET, SHADOW_TMAX

F32 = np.float32


# ---- the derived tables ---------------------------------------------------------------------------------------------------------------
def bases(ranges, object_ids):
    """(n, 2) int32: {first_tri(o_k), light_base[k] - first_light(o_k)}, light_base the exclusive prefix sum of num_lights(o_k)."""
    r = np.asarray(ranges, np.int64)[np.asarray(object_ids)]
    light_base = np.cumsum(r[:, 3]) - r[:, 3]
    return np.stack([r[:, 0], light_base - r[:, 2]], 1).astype(np.int32)


def light_owner(ranges, object_ids):
    return np.repeat(np.arange(len(object_ids)), np.asarray(ranges)[np.asarray(object_ids), 3]).astype(np.int32)


def slot_of(instances):
    """slot_of[k] = the leaf-order slot of instance k (instances: INSTANCE records in leaf order)."""
    ids = instances["instance_id"] & 0x7FFFFFFF
    out = np.zeros(len(ids), np.int32)
    out[ids] = np.arange(len(ids))
    return out


def map_points(m, p):
    """Rows of p (n, 3) under the matrices m (n, 12): ((m0 x + m1 y) + m2 z) + m3 per row, float32."""
    m = np.asarray(m, F32).reshape(-1, 3, 4)
    p = np.asarray(p, F32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return (((m[:, :, 0] * x + m[:, :, 1] * y) + m[:, :, 2] * z) + m[:, :, 3]).astype(F32)


def map_normals(w, n):
    """N(n) of rows n (n, 3) under world_to_object matrices w (n, 12): n times the transpose of w's 3 x 3 part, float32."""
    w = np.asarray(w, F32).reshape(-1, 3, 4)
    n = np.asarray(n, F32)
    return ((w[:, 0, :3] * n[:, 0:1] + w[:, 1, :3] * n[:, 1:2]) + w[:, 2, :3] * n[:, 2:3]).astype(F32)


def normalized(v):
    """v * (1 / sqrt((x x + y y) + z z)), float32: the shader's normalize()."""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        return (v * (F32(1) / np.sqrt(l2))[:, None]).astype(F32)


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)


def world_lights(object_lights, ranges, transforms, object_ids):
    """The world light table (scene.LIGHT): light light_base[k] + j is object light first_light(o_k) + j under instance k."""
    t = np.asarray(transforms, F32).reshape(-1, 12)
    w, _ = M.invert(t)
    owner = light_owner(ranges, object_ids)
    src = np.arange(len(owner)) - bases(ranges, object_ids)[owner, 1]
    out = np.array(np.asarray(object_lights, LIGHT)[src])
    m = t[owner]
    for name in ("v0", "v1", "v2"):
        out[name][:, :3] = map_points(m, out[name][:, :3])
    c = cross(out["v1"][:, :3] - out["v0"][:, :3], out["v2"][:, :3] - out["v0"][:, :3])
    with np.errstate(all="ignore"):
        l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        out["inv_area"] = F32(1) / (F32(0.5) * l)
    out["n"] = normalized(map_normals(w[owner], out["n"]))
    return out


# ---- the scene, baked flat ------------------------------------------------------------------------------------------------------------
class Baked:
    @property
    def num_tris(self):
        return len(self.indices)


def baked(scene, ranges, transforms, object_ids):
    """The flat scene whose tables shade, through the flat shader, exactly as the instanced one: triangle q = tri_base[k] + p is
    triangle p of instance k's object (tri_base: the exclusive prefix sum of the instances' triangle counts), with three fresh
    vertices 3q, 3q + 1, 3q + 2: positions by the corner rule, normals N(n_i) (not normalised), face normal normalize(N(fn)),
    texture coordinates copied, light ids and lights the world ones.  No hierarchy (`tri_base` maps a hit to q)."""
    ranges, object_ids = np.asarray(ranges, np.int64), np.asarray(object_ids)
    t = np.asarray(transforms, F32).reshape(-1, 12)
    w, _ = M.invert(t)
    b = bases(ranges, object_ids)
    counts = ranges[object_ids, 1]
    out = Baked()
    out.tri_base = (np.cumsum(counts) - counts).astype(np.int64)
    inst = np.repeat(np.arange(len(object_ids)), counts)                                   # instance of every baked triangle
    gprim = np.concatenate([np.arange(ranges[o, 0], ranges[o, 0] + ranges[o, 1]) for o in object_ids])
    ind = np.asarray(scene.indices)[gprim]
    corners = ind[:, :3].reshape(-1)                                                        # object vertex of every baked vertex
    vinst = np.repeat(inst, 3)
    out.vertices = np.array(np.asarray(scene.vertices, F32)[corners])
    out.vertices[:, :3] = map_points(t[vinst], out.vertices[:, :3])
    out.normals = np.array(np.asarray(scene.normals, F32)[corners])
    out.normals[:, :3] = map_normals(w[vinst], out.normals[:, :3])
    out.face_normals = np.array(np.asarray(scene.face_normals, F32)[gprim])
    out.face_normals[:, :3] = normalized(map_normals(w[inst], out.face_normals[:, :3]))
    out.texcoords = np.array(np.asarray(scene.texcoords, F32)[corners])
    q = np.arange(len(gprim), dtype=np.int32)
    out.indices = np.stack([3 * q, 3 * q + 1, 3 * q + 2, ind[:, 3]], 1).astype(np.int32)
    emissive = np.asarray(scene.materials)["emissive"][ind[:, 3]] != 0
    out.light_ids = np.where(emissive, np.asarray(scene.light_ids)[gprim] + b[inst, 1], 0).astype(np.int32)
    out.lights = world_lights(scene.lights, ranges, t, object_ids)
    out.materials, out.textures, out.texels = scene.materials, scene.textures, scene.texels
    out.nodes, out.tris = np.zeros(0, F.NODE2), np.zeros(0, F.TRI1)
    return out


def with_flat_bvh(b, max_leaf=2):
    """`b` with a flat BVH2 over its own triangles (lbvh_model.build: geom_id = the material), for oracle.render."""
    b.nodes, b.tris, info = L.build(b.vertices, b.indices, max_leaf)
    assert info[2] == 0
    return b


# ---- the two-level hierarchy of a scene -------------------------------------------------------------------------------------------------
def object_bvhs(scene, ranges, max_leaf=2):
    """(nodes, tris, table): every object's hierarchy as the device builder writes it (lbvh_model.build over its index range: prim ids
    are object-local), packed by instance_model.pack."""
    built = []
    for first, n, _, _ in np.asarray(ranges):
        nodes, tris, info = L.build(scene.vertices, np.asarray(scene.indices)[first:first + n], max_leaf)
        assert info[2] == 0
        built.append((nodes, tris))
    return M.pack(built)


def tlas_of(nodes, table, transforms, object_ids):
    """(tlas nodes, instances in leaf order, info) as the scene builds them: ids 0 ... n - 1, max_leaf 1."""
    return M.build_tlas(nodes, table, M.descriptors(transforms, object_ids), 1)


# ---- a frame ----------------------------------------------------------------------------------------------------------------------------
class Frame:
    """film (h, w, 3) float32, counts [primary rays, shadow rays], and per bounce what was traced: `primary` and `shadow` lists of
    (rays RAY1, pixel ids, hits HIT1, instance ids) as instance_model.trace answered them (shadow: and the rays' colours), and
    `vertices`: per bounce (ORACLE_VERTEX records with prim = the BAKED triangle, pixel ids, instance ids, object-local prim ids) of
    the hits that were shaded."""


def frame(scene, ranges, transforms, object_ids, hierarchy, cam, iter_, spp, max_path_len, width, height):
    """One frame of the instanced scene: shade_fixtures.walk_paths with instance_model.trace in place of the flat traversal and
    oracle.shade_vertices over baked(...) with prim = tri_base[instance] + the hit's object-local prim id.  hierarchy: (nodes, tris,
    table) of object_bvhs, or the device's own arrays.  Per pixel the additions happen in oracle_render's order, in float32."""
    nodes, tris, table = hierarchy
    tlas, inst, info = tlas_of(nodes, table, transforms, object_ids)
    assert info[2] == 0
    flat = baked(scene, ranges, transforms, object_ids)
    y, x, sample = [a.reshape(-1) for a in np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")]
    rnd, d = O.emit_samples(cam, iter_, width, height, x, y, sample)
    n = len(rnd)
    v = np.zeros(n, O.ORACLE_VERTEX)
    v["org"] = np.asarray(cam["eye"], "<f4"); v["dir"] = d; v["rnd"] = rnd; v["contrib"] = 1.0
    path = np.arange(n)
    tmin = np.zeros(n, "<f4")
    inv_spp = F32(1.0) / F32(spp)
    adds = [[] for _ in range(n)]
    out = Frame()
    out.primary, out.shadow, out.vertices, out.counts = [], [], [], [0, 0]
    out.tlas, out.instances, out.baked = tlas, inst, flat
    while len(v):
        rays = F.make_rays(v["org"], v["dir"], tmin, FLT_MAX_REF)
        hits, ids = M.trace(O, tlas, inst, nodes, tris, rays)
        out.primary.append((rays, path // spp, hits, ids)); out.counts[0] += len(rays)
        hit = hits["tri_id"] >= 0
        v, path, hits, ids = v[hit], path[hit], hits[hit], ids[hit]
        if not len(v):
            break
        v["prim"] = flat.tri_base[ids] + hits["tri_id"]; v["t"] = hits["t"]; v["u"] = hits["u"]; v["v"] = hits["v"]
        out.vertices.append((v.copy(), path // spp, ids, hits["tri_id"].copy()))
        o = O.shade_vertices(flat, v, max_path_len)
        sh = o["shadow"] != 0
        srays = F.make_rays(o["s_org"][sh], o["s_dir"][sh], RAY_OFFSET, SHADOW_TMAX)
        occl, oids = M.trace(O, tlas, inst, nodes, tris, srays, any_hit=True)
        out.shadow.append((srays, path[sh] // spp, occl, oids, o["s_color"][sh])); out.counts[1] += len(srays)
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
CUBE_OBJ = """mtllib parts.mtl
v -0.5 -0.5 -0.5
v 0.5 -0.5 -0.5
v 0.5 0.5 -0.5
v -0.5 0.5 -0.5
v -0.5 -0.5 0.5
v 0.5 -0.5 0.5
v 0.5 0.5 0.5
v -0.5 0.5 0.5
usemtl mix
f 1 4 3
f 1 3 2
f 5 6 7
f 5 7 8
f 1 2 6
f 1 6 5
f 3 4 8
f 3 8 7
f 2 3 7
f 2 7 6
f 1 5 8
f 1 8 4
"""
QUAD_OBJ = """mtllib parts.mtl
v -0.5 0 -0.5
v 0.5 0 -0.5
v 0.5 0 0.5
v -0.5 0 0.5
usemtl glow
f 1 2 3
f 1 3 4
"""
PARTS_MTL = "newmtl mix\nKd 0.5 0.3 0.2\nKs 0.4 0.4 0.4\nNs 20\nnewmtl glow\nKd 0 0 0\nKe 6 5 3\n"


def scene_objects(golden, tmp):
    """[Cornell box, cube, emissive quad] as scene.Scene objects (converted into directory `tmp`)."""
    from rodent_amd import scene as S
    (tmp / "parts.mtl").write_text(PARTS_MTL)
    (tmp / "cube.obj").write_text(CUBE_OBJ)
    (tmp / "quad.obj").write_text(QUAD_OBJ)
    return [S.convert(golden / "cornell_box.obj", tmp / "cornell.rscene"), S.convert(tmp / "cube.obj", tmp / "cube.rscene"),
            S.convert(tmp / "quad.obj", tmp / "quad.rscene")]


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def placements(moved=False):
    """(transforms (7, 12) float32, object ids): the box under the identity; the cube under an oblique rotation with a non-uniform
    scale, under a mirroring matrix (negative determinant), and twice under ONE matrix (equal t: the <= rule across instances); the
    quad (its corners wind so that it emits downwards) under a rotation with one scale and under a MIRRORING matrix with another: the
    cross product of the mirrored corners points up, N(n) keeps pointing down.  moved: the cubes and quads somewhere else."""
    def place(linear, translation):
        t = np.zeros((3, 4)); t[:, :3] = linear; t[:, 3] = translation
        return t
    s = 1.0 if not moved else -1.0
    t = [place(np.eye(3), (0, 0, 0)),
         place(_rotation((1, 2, 0.5), 0.9 + 0.4 * moved) @ np.diag([0.35, 0.5, 0.25]), (-0.45 * s, 0.45, 0.3)),
         place(_rotation((0, 1, 0), 0.5) @ np.diag([-0.3, 0.3, 0.3]), (0.5 * s, 0.25, 0.45)),
         place(_rotation((0.2, 1, 0.1), -0.4) @ np.diag([0.3, 0.2, 0.3]), (0.05, 1.2 + 0.1 * moved, -0.2)),
         None,
         place(_rotation((0, 1, 0), 0.3) @ np.diag([0.5, 1.0, 0.5]), (-0.5 * s, 1.6, 0.2)),
         place(_rotation((0, 0, 1), 0.15) @ np.diag([-0.25, 1.0, 0.35]), (0.55 * s, 1.4, -0.3))]
    t[4] = t[3]
    return np.asarray(t).reshape(7, 12).astype(F32), np.array([0, 1, 1, 1, 1, 2, 2], np.int32)


W, H, SPP, MAXLEN = 96, 64, 2, 6
