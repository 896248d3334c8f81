"""CPU model of geometry that deforms inside the objects of an instanced scene (rodent_hip_scene_deform_device, include/rodent_render.h;
rodent_hip_refit_objects, include/rodent_instances.h) in numpy, over the models that exist: scene_update_model (the rules of a moved
flat scene), refit_model (the refit of one hierarchy) and instanced_scene_model (the derived tables and the frame).

  tables      the scene's object-space tables after a deform: scene_update_model's rules restricted to the deforming set D
  hierarchy   the packed hierarchy: refit_model.refit per listed object of the packed original, every other object as it is
  frame       instanced_scene_model.frame of the deformed scene
"""
from __future__ import annotations

import copy

import numpy as np

import instanced_scene_model as IM
import refit_model as R
import scene_update_model as SU

F32 = np.float32


def in_set(ranges, objects, num_tris):
    """Boolean mask over the index table: the triangles of D's ranges."""
    mask = np.zeros(num_tris, bool)
    for o in objects:
        mask[ranges[o][0]: ranges[o][0] + ranges[o][1]] = True
    return mask


def tables(scene, ranges, objects, vertices, normals=None):
    """A copy of `scene` (the concatenated tables, duck-typed like scene.Scene) after D = `objects` took `vertices` (the whole table;
    rows no object of D names equal the scene's): face normals of D's triangles; vertex normals of the vertices D's triangles name,
    summed over ALL triangles that name them with the static ones' stored face normals (or `normals`, the whole table); the object
    lights of D's light ranges bound to the lowest emissive triangle that names them.  Everything else keeps its bytes.  `tri_shade`:
    the gathered records, D's rows from the new tables, the others from the old ones."""
    ranges = np.asarray(ranges)
    ix = np.asarray(scene.indices, np.int32).reshape(-1, 4)
    nv = len(scene.vertices)
    d_tris = in_set(ranges, objects, len(ix))
    out = copy.copy(scene)
    out.vertices = np.ascontiguousarray(vertices, F32).reshape(nv, 4).copy()
    out.face_normals = np.array(scene.face_normals, F32)
    out.face_normals[d_tris] = SU.face_normals(out.vertices, ix)[d_tris]
    if normals is None:
        d_verts = np.zeros(nv, bool)
        d_verts[ix[d_tris, :3].reshape(-1)] = True
        out.normals = np.array(scene.normals, F32)
        out.normals[d_verts] = SU.smooth_normals(out.face_normals, ix, nv)[d_verts]
    else:
        out.normals = np.ascontiguousarray(normals, F32).reshape(nv, 4).copy()
    out.lights = np.array(scene.lights)
    moved = SU.light_records(out.lights, out.vertices, ix, scene.materials, scene.light_ids)
    for o in objects:
        first, n = ranges[o][2], ranges[o][3]
        out.lights[first: first + n] = moved[first: first + n]
    out.tri_shade = SU.tri_shade(np.asarray(scene.face_normals, F32), np.asarray(scene.normals, F32), ix)
    out.tri_shade[d_tris] = SU.tri_shade(out.face_normals, out.normals, ix)[d_tris]
    return out


def hierarchy(packed, ranges, objects, vertices, indices):
    """(nodes, tris, table, info): the packed hierarchy `packed` = (nodes, tris, table) with every listed object refitted alone
    (refit_model.refit over its own rows of the index table), and the info words summed over the listed objects."""
    nodes, tris, table = packed[0].copy(), packed[1].copy(), packed[2]
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    info = np.zeros(4, np.int32)
    for o in objects:
        row, (first, n) = table[o], ranges[o][:2]
        ns = slice(int(row["node_offset"]), int(row["node_offset"] + row["num_nodes"]))
        ts = slice(int(row["tri_offset"]), int(row["tri_offset"] + row["num_tris"]))
        nodes[ns], tris[ts], words = R.refit(nodes[ns], tris[ts], vertices, ix[first: first + n])
        info[:2] += words[:2]; info[2] |= words[2]
    return nodes, tris, table, info


def frame(deformed, ranges, transforms, object_ids, refitted, cam, iter_, spp, max_path_len, width, height):
    """instanced_scene_model.frame of the deformed scene (`deformed`: tables(...), `refitted`: hierarchy(...))."""
    return IM.frame(deformed, ranges, transforms, object_ids, refitted[:3], cam, iter_, spp, max_path_len, width, height)


def shear_objects(scene, ranges, objects, kx=0.25, kz=0.1, ky=0.2):
    """scene_update_model.shear (x += kx y, z += kz y), then y += ky x (a flat object in a plane y = const moves too), applied in fp32
    to the vertices D's triangles name; every other row as it is."""
    ix = np.asarray(scene.indices, np.int32).reshape(-1, 4)
    named = np.unique(ix[in_set(np.asarray(ranges), objects, len(ix)), :3])
    v = np.array(scene.vertices, F32).reshape(-1, 4).copy()
    moved = SU.shear(v[named], kx, kz)
    moved[:, 1] = moved[:, 1] + F32(ky) * moved[:, 0]
    v[named] = moved
    return v
