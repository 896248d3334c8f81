"""CPU model of the device scene update (rodent_hip_scene_refit_device, rodent_amd/csrc/render_update.h) in numpy.

It restates the rules of include/rodent_render.h ("moved geometry that is already on the device") and predicts the bytes of every table
the scene derives from positions: face normals, smooth vertex normals, light records, the gathered tri_shade records and the LDS top
images.  fp32 throughout, every operation rounded on its own (numpy float32 arithmetic is exactly that); sums are taken in the stated
order.  The hierarchy's own bytes are tests/refit_model.py's.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
LDS_TAG = 0x40000000            # traversal_device.h kLdsTag
NODE_BYTES = 64


def _cross_of_corners(vertices, indices):
    """(c, v0, v1, v2): c = (v1 - v0) x (v2 - v0) per triangle, host/vec.h's cross."""
    v = np.asarray(vertices, F32).reshape(-1, 4)
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    v0, v1, v2 = (v[ix[:, k], :3] for k in range(3))
    a, b = v1 - v0, v2 - v0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)
    return c, v0, v1, v2


def _length(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def face_normals(vertices, indices):
    """(num_tris, 4) float32: c * (1 / |c|), w = 0; NaN for a degenerate triangle."""
    with np.errstate(all="ignore"):
        c, *_ = _cross_of_corners(vertices, indices)
        inv = F32(1.0) / _length(c)
        out = np.zeros((len(c), 4), F32)
        out[:, :3] = c * inv[:, None]
    return out


def incidence(indices, num_vertices):
    """(first, tri): the corners naming vertex v are tri[first[v]:first[v + 1]], in ascending (triangle, corner) order."""
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    corners = ix[:, :3].reshape(-1)                                   # corner 3 t + k: ascending (t, k)
    order = np.argsort(corners, kind="stable")
    first = np.zeros(num_vertices + 1, np.int64)
    np.add.at(first, corners.astype(np.int64) + 1, 1)
    return np.cumsum(first), (order // 3).astype(np.int64)


def smooth_normals(face_normals_, indices, num_vertices):
    """(num_vertices, 4) float32: per vertex the face normals of its corners summed in list order, then the loader's normalisation."""
    first, tri = incidence(indices, num_vertices)
    count = first[1:] - first[:-1]
    s = np.zeros((num_vertices, 3), F32)
    with np.errstate(all="ignore"):
        for rank in range(int(count.max()) if num_vertices else 0):  # one more corner of every vertex that has one
            on = np.nonzero(count > rank)[0]
            s[on] = s[on] + face_normals_[tri[first[on] + rank], :3]
        l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        keep = l2 > np.finfo(F32).eps                                 # false for a NaN
        out = np.zeros((num_vertices, 4), F32)
        out[:, 1] = 1.0
        inv = F32(1.0) / np.sqrt(l2[keep])
        out[keep, :3] = s[keep] * inv[:, None]
    return out


def light_triangles(indices, materials, light_ids, num_lights):
    """Per light the lowest emissive triangle whose light id names it, -1 for none."""
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    out = np.full(num_lights, -1, np.int64)
    emissive = np.asarray(materials["emissive"])[ix[:, 3]] != 0
    for t in np.nonzero(emissive)[0][::-1]:
        if 0 <= light_ids[t] < num_lights:
            out[light_ids[t]] = t
    return out


def light_records(lights, vertices, indices, materials, light_ids):
    """The light table after the move: bound lights get their triangle's corners, normal and 1 / area; everything else stays."""
    lights = lights.copy()
    bound = light_triangles(indices, materials, light_ids, len(lights))
    k = np.nonzero(bound >= 0)[0]
    if len(k) == 0:
        return lights
    with np.errstate(all="ignore"):
        c, v0, v1, v2 = _cross_of_corners(vertices, np.asarray(indices, np.int32).reshape(-1, 4)[bound[k]])
        l = _length(c)
        for name, val in (("v0", v0), ("v1", v1), ("v2", v2)):
            field = lights[name]
            field[k, :3] = val
            lights[name] = field
        n = lights["n"]; n[k] = c * (F32(1.0) / l)[:, None]; lights["n"] = n
        ia = lights["inv_area"]; ia[k] = F32(1.0) / (F32(0.5) * l); lights["inv_area"] = ia
    return lights


def tri_shade(face_normals_, normals, indices):
    """(num_tris, 12) float32: the face normal's x y z, then the three corners' vertex normals."""
    ix = np.asarray(indices, np.int32).reshape(-1, 4)
    return np.concatenate([face_normals_[:, :3]] + [normals[ix[:, k], :3] for k in range(3)], 1).astype(F32)


def top_image(nodes, capacity):
    """(capacity, 16) int32: the LDS top image, level by level.  The slot of child j of the i-th node of a level is the count of slots
    taken so far plus the inner children of the level's earlier nodes (plus one for j = 1 when child 0 is inner); a child gets it only
    while it is below the capacity."""
    image = np.zeros((capacity, 16), np.int32)
    words = nodes.view(np.int32).reshape(-1, 16)
    level = np.array([1], np.int64)                                   # 1-based node ids of the level, in slot order
    begin = 0
    while len(level):
        rec = words[level - 1].copy()
        child = rec[:, 12:14].astype(np.int64)
        inner = child > 0
        per_node = inner.sum(1)
        before = begin + len(level) + np.cumsum(per_node) - per_node  # slots taken before this node's children
        slot = np.stack([before, before + inner[:, 0]], 1)
        linked = inner & (slot < capacity)
        rec[:, 12:14] = np.where(linked, LDS_TAG + slot * NODE_BYTES, child).astype(np.int32)
        rec[:, 14] = level
        rec[:, 15] = 0
        image[begin: begin + len(level)] = rec
        begin += len(level)
        level = child[linked]                                         # row-major: child 0 before child 1, node by node
    return image


def shear(vertices, kx=0.25, kz=0.1):
    """The move of the scene update tests: x += kx y, z += kz y in fp32; w stays."""
    v = np.array(vertices, F32).reshape(-1, 4).copy()
    v[:, 0] = v[:, 0] + F32(kx) * v[:, 1]
    v[:, 2] = v[:, 2] + F32(kz) * v[:, 1]
    return v


def indexed_soup(n, seed, twice=False):
    """(vertices, indices, light_ids, lights): n triangles over a shared vertex pool, material 1 (the emitter) for every fifth triangle.
    From 140 triangles on, the first 70 form a fan around vertex 0; the pool's last vertex is named by nobody; with `twice`, triangle 1
    names one vertex twice (degenerate: its face normal is NaN).  Lights: one per emissive triangle in order, except that the last
    emissive triangle names light 0 again (light 0 stays bound to the lowest), plus one light that no triangle names."""
    rng = np.random.default_rng(seed)
    nv = max(3, n // 2 + 3)
    v = np.zeros((nv + 1, 4), F32)
    v[:, :3] = rng.uniform(-10, 10, (nv + 1, 3)).astype(F32)
    ix = np.zeros((n, 4), np.int32)
    for t in range(n):
        ix[t, :3] = rng.choice(nv, 3, replace=False)
    if n >= 140:
        for t in range(70):
            a, b = rng.choice(np.arange(1, nv), 2, replace=False)
            ix[t, :3] = (0, a, b)
    if twice:
        ix[1, 2] = ix[1, 0]
    ix[::5, 3] = 1
    emitters = np.nonzero(ix[:, 3] == 1)[0]
    light_ids = np.zeros(n, np.int32)
    light_ids[emitters] = np.arange(len(emitters))
    if len(emitters) > 2:
        light_ids[emitters[-1]] = 0
    from rodent_amd.scene import LIGHT
    lights = np.zeros(len(emitters) + 1, LIGHT)
    lights["color"][:, :3] = rng.uniform(1, 9, (len(lights), 3)).astype(F32)
    lights["v0"][-1] = (1, 2, 3, 4); lights["v1"][-1] = (5, 6, 7, 8); lights["v2"][-1] = (9, 10, 11, 12)
    lights["n"][-1] = (0, 0, 1); lights["inv_area"][-1] = 0.5
    return v, ix, light_ids, lights
