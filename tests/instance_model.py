"""CPU model of instanced scenes (include/rodent_instances.h; rodent_amd/csrc/build_tlas.h, traversal_instanced.h) in numpy.

It restates the header's rules and predicts the device's bytes:
  invert, world_box   the fp64 cofactor inverse rounded once, the widened world box of an object box under a 3 x 4 matrix
  build_tlas          the instance stage, then lbvh_model's morton_codes / karras / emit over the instances' boxes
  trace               a per-ray walk of the TLAS by the reference's step; an instance is entered by handing the transformed ray, with the
                      current tmax, to oracle.binding.traverse: the object's own traversal is the oracle's, bit for bit
  peak                every ray's stack peak P: the TLAS entries held when an instance is entered + that object's peak for the ray
numpy float32 / float64 arithmetic is correctly rounded, operation by operation, like the kernels under -ffp-contract=off; the one fused
operation, the slab test's fma, is computed exactly (fma32).
"""
from __future__ import annotations

import numpy as np

import lbvh_model as L
from rodent_amd import formats as F

BAD_OBJECT, BAD_TRANSFORM = 8, 16
F32, F64 = np.float32, np.float64
FLT_MAX = F32(3.4028234664e+38)


def pack(objects):
    """(nodes, tris, table OBJECT) of a list of (nodes NODE2, tris TRI1) pairs: concatenation, no id rewritten."""
    table = np.zeros(len(objects), F.OBJECT)
    table["num_nodes"] = [len(n) for n, _ in objects]
    table["num_tris"] = [len(t) for _, t in objects]
    table["node_offset"] = np.cumsum(table["num_nodes"]) - table["num_nodes"]
    table["tri_offset"] = np.cumsum(table["num_tris"]) - table["num_tris"]
    return np.concatenate([n for n, _ in objects]), np.concatenate([t for _, t in objects]), table


def descriptors(transforms, object_ids, instance_ids=None):
    """The INSTANCE_DESC array of (n, 12) / (n, 3, 4) transforms."""
    t = np.asarray(transforms, F32).reshape(len(transforms), 12)
    d = np.zeros(len(t), F.INSTANCE_DESC)
    d["object_to_world"], d["object"] = t, object_ids
    d["instance_id"] = np.arange(len(t)) if instance_ids is None else instance_ids
    return d


def invert(m):
    """world_to_object (n, 12) float32 of object_to_world (n, 12), and per matrix whether it raises BAD_TRANSFORM."""
    m = np.asarray(m, F32).reshape(-1, 12)
    a, b, c, tx, d, e, f, ty, g, h, i, tz = (m[:, k].astype(F64) for k in range(12))
    with np.errstate(all="ignore"):
        c0, c1, c2 = e * i - f * h, f * g - d * i, d * h - e * g
        det = (a * c0 + b * c1) + c * c2
        r = F64(1.0) / det
        q = [[c0 * r, (c * h - b * i) * r, (b * f - c * e) * r],
             [c1 * r, (a * i - c * g) * r, (c * d - a * f) * r],
             [c2 * r, (b * g - a * h) * r, (a * e - b * d) * r]]
        w = np.empty((len(m), 12), F32)
        for k in range(3):
            for j in range(3):
                w[:, 4 * k + j] = q[k][j].astype(F32)
            w[:, 4 * k + 3] = (-((q[k][0] * tx + q[k][1] * ty) + q[k][2] * tz)).astype(F32)
    bad = ~np.isfinite(m).all(1) | (det == 0) | ~np.isfinite(det) | ~np.isfinite(w).all(1)
    return w, bad


def object_box(root):
    """(lo[3], hi[3]) of an object: the union of its root node's two child boxes."""
    b = root["bounds"]
    return np.fmin(b[0:6:2], b[6:12:2]), np.fmax(b[1:6:2], b[7:12:2])


def world_box(m, olo, ohi):
    """The widened world boxes (n, 6: lo_x hi_x lo_y hi_y lo_z hi_z) of object boxes olo / ohi (n, 3) under matrices m (n, 12)."""
    m = np.asarray(m, F32).reshape(-1, 3, 4)
    olo, ohi = np.asarray(olo, F32).reshape(-1, 3), np.asarray(ohi, F32).reshape(-1, 3)
    box = np.empty((len(m), 6), F32)
    with np.errstate(all="ignore"):
        mag = np.fmax(np.abs(olo), np.abs(ohi))
        for a in range(3):
            r = m[:, a]
            mn, mx = np.full(len(m), np.inf, F32), np.full(len(m), -np.inf, F32)
            for corner in range(8):
                x, y, z = (np.where(corner >> k & 1, ohi[:, k], olo[:, k]) for k in range(3))
                v = ((r[:, 0] * x + r[:, 1] * y) + r[:, 2] * z) + r[:, 3]
                mn, mx = np.fmin(mn, v), np.fmax(mx, v)
            e = F32(2.0 ** -21) * (((np.abs(r[:, 0]) * mag[:, 0] + np.abs(r[:, 1]) * mag[:, 1]) + np.abs(r[:, 2]) * mag[:, 2])
                                   + np.abs(r[:, 3]))
            box[:, 2 * a], box[:, 2 * a + 1] = (mn + F32(0)) - e, (mx + F32(0)) + e
    return box


def build_tlas(nodes, table, descs, max_leaf=1):
    """(tlas nodes NODE2, instances INSTANCE in leaf order, info int32[4]) as rodent_hip_build_tlas writes them."""
    assert 1 <= max_leaf <= 8 and 1 <= len(descs) <= 1 << 22 and len(table) >= 1
    flags = 0
    obj = descs["object"].astype(np.int64)
    outside = (obj < 0) | (obj >= len(table))
    if outside.any():
        flags |= BAD_OBJECT
    ob = table[np.where(outside, 0, obj)]
    m = descs["object_to_world"]
    w, bad = invert(m)
    if bad.any():
        flags |= BAD_TRANSFORM
    roots = nodes[ob["node_offset"]]["bounds"]
    olo, ohi = np.fmin(roots[:, 0:6:2], roots[:, 6:12:2]), np.fmax(roots[:, 1:6:2], roots[:, 7:12:2])
    box = world_box(m, olo, ohi)
    with np.errstate(all="ignore"):
        points = box[:, 0::2] + box[:, 1::2]
        codes = L.morton_codes(points)
    order = np.lexsort((np.arange(len(codes)), codes))
    # emit() marks leaf ends in a Tri1 array's prim_id: the instance ids ride through it
    t_nodes, marked, info = L.emit(codes[order], box[order], np.zeros(len(order), F.TRI1),
                                   (descs["instance_id"][order] & 0x7FFFFFFF).astype(np.int64), max_leaf)
    inst = np.zeros(len(order), F.INSTANCE)
    inst["world_to_object"] = w[order]
    inst["node_offset"], inst["tri_offset"] = ob["node_offset"][order], ob["tri_offset"][order]
    inst["instance_id"] = marked["prim_id"]
    info[2] = flags
    return t_nodes, inst, info


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------------
def flat_object(z=0.5):
    """(nodes, tris) of a quad in the plane z = const under a single-leaf root: an object whose box is flat on one axis."""
    tris = np.zeros(2, F.TRI1)
    corners = F32([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]])
    for k, (a, b, c) in enumerate(((0, 1, 2), (0, 2, 3))):
        tris[k]["v0"], tris[k]["e1"], tris[k]["e2"] = corners[a], corners[a] - corners[b], corners[c] - corners[a]
    tris["prim_id"] = [0, 1 | -(1 << 31)]
    return L.single_leaf(F32([-1, 1, -1, 1, z, z])), tris


def seeded_transforms(n, seed, extent, num_objects):
    """(transforms (n, 12) float32, object ids) of n seeded instances: a rotation about a random axis times a non-uniform scale in
    (0.5, 2), every third one mirrored (a negative determinant), translations in [-extent, extent]^3.  Instance 1 coincides with
    instance 0 (same object, same matrix); instance 2 is an axis-aligned placement of the LAST object (with flat_object there: a world
    box that is flat on one axis up to its widening)."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(n, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0, 2 * np.pi, n)
    k = np.zeros((n, 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = (-axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0],
                                                                               -axis[:, 1], axis[:, 0])
    rot = np.eye(3) + np.sin(angle)[:, None, None] * k + (1 - np.cos(angle))[:, None, None] * (k @ k)
    scale = rng.uniform(0.5, 2.0, (n, 3))
    scale[::3, 0] *= -1
    t = np.zeros((n, 3, 4))
    t[:, :, :3] = rot * scale[:, None, :]
    t[:, :, 3] = rng.uniform(-extent, extent, (n, 3))
    obj = rng.integers(0, num_objects, n).astype(np.int32)
    if n >= 2:
        t[1], obj[1] = t[0], obj[0]
    if n >= 3:
        t[2, :, :3], obj[2] = np.diag([1.5, 0.75, 2.0]), num_objects - 1
    return t.reshape(n, 12).astype(F32), obj


# ---- traversal ------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum gives its
    error), and rounding THAT to float32 rounds the exact value once."""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.atleast_1d(p + c)
        t = s - p
        err = (p - (s - t)) + (c - t)
        odd = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32).reshape(p.shape)


def make_ray(org, direction):
    """(inv_dir, inv_org) by intersection.impala:88-99: safe_rcp, then -(org * inv_dir)."""
    with np.errstate(all="ignore"):
        tiny = np.abs(direction) < F32(1e-8)
        idir = np.where(tiny, np.copysign(FLT_MAX, direction), F32(1) / np.where(tiny, F32(1), direction)).astype(F32)
        return idir, -(org * idir)


def _tlas_slabs(tlas, rays):
    """Per (ray, node, child): the entry distance and the exit distance without the ray's tmax (NaN -> +inf: fminf drops a NaN)."""
    org, d = rays["org"], rays["dir"]
    idir, iorg = make_ray(org, d)
    b = tlas["bounds"].reshape(len(tlas), 2, 3, 2)                                    # node, child, axis, lo / hi
    t = fma32(idir[:, None, None, :, None], b[None], iorg[:, None, None, :, None])     # ray, node, child, axis, lo / hi
    with np.errstate(all="ignore"):
        near, far = np.fmin(t[..., 0], t[..., 1]), np.fmax(t[..., 0], t[..., 1])
        entry = np.fmax(np.fmax.reduce(near, axis=-1), rays["tmin"][:, None, None])
        far = np.fmin.reduce(far, axis=-1)
    return entry, np.where(np.isnan(far), np.inf, far)


def _object_rays(inst, rays):
    """Per (ray, instance): org' and dir' in the instance's object space."""
    w = inst["world_to_object"].reshape(1, len(inst), 3, 4)
    o, d = rays["org"][:, None, :], rays["dir"][:, None, :]
    with np.errstate(all="ignore"):
        org = ((w[..., 0] * o[..., 0:1] + w[..., 1] * o[..., 1:2]) + w[..., 2] * o[..., 2:3]) + w[..., 3]
        direction = (w[..., 0] * d[..., 0:1] + w[..., 1] * d[..., 1:2]) + w[..., 2] * d[..., 2:3]
    return org.astype(F32), direction.astype(F32)


# Three decisions of the walk, as functions of their own so that a test can replace one and see the expectations change
# (tests/test_instance_edge_fixtures.py).
def _child0_first(entry0, entry1):
    return entry0 < entry1                                              # strict <: a tie goes into child 1 (mapping_gpu.impala:128-129)


def _instance_tmax(tmax, hit_inst):
    return F32(tmax)                                                    # the current tmax as it is: acceptance stays <= across instances


def _miss_t(tmax):
    return tmax                                                         # the ray's tmax bit for bit, a signalling NaN included


def _walk(oracle, tlas, inst, nodes, tris, rays, any_hit, want_peak):
    rays = np.ascontiguousarray(rays)
    hits = np.zeros(len(rays), F.HIT1)
    ids = np.full(len(rays), -1, np.int32)
    peaks = np.zeros(len(rays), np.int64)
    child = tlas["child"].tolist()
    inst_id = inst["instance_id"].tolist()
    block = max(1, (1 << 18) // max(len(tlas), len(inst)))
    one = np.zeros(1, F.RAY1)
    for start in range(0, len(rays), block):
        part = rays[start:start + block]
        entry, far = _tlas_slabs(tlas, part)
        o_org, o_dir = _object_rays(inst, part)
        entry, far = entry.tolist(), far.tolist()
        for k in range(len(part)):
            tmax, hit, hit_inst, peak = float(part[k]["tmax"]), (-1, _miss_t(part[k]["tmax"]), F32(0), F32(0)), -1, 0
            mem, ptr, top, done = {0: 0}, 0, 1, False
            while top != 0 and not done:
                n = top - 1
                h = [entry[k][n][c] <= min(far[k][n][c], tmax) and child[n][c] != 0 for c in (0, 1)]
                if not h[0] and not h[1]:
                    top = mem[ptr]; ptr -= 1
                elif h[0] and h[1]:
                    c0first = _child0_first(entry[k][n][0], entry[k][n][1])
                    top = child[n][0 if c0first else 1]
                    ptr += 1; mem[ptr] = child[n][1 if c0first else 0]
                else:
                    top = child[n][0 if h[0] else 1]
                while top < 0:                                       # a leaf: its continuation stays on the stack (ptr entries held)
                    j = ~top
                    while True:
                        one["org"], one["dir"], one["tmin"], one["tmax"] = o_org[k, j], o_dir[k, j], part[k]["tmin"], _instance_tmax(tmax, hit_inst)
                        on, ot = nodes[inst["node_offset"][j]:], tris[inst["tri_offset"][j]:]
                        if want_peak:
                            peak = max(peak, ptr + int(oracle.ray_depths(on, ot, one, any_hit=any_hit)[0]))
                        got = oracle.traverse(2, on, ot, one, any_hit=any_hit)[0][0]
                        if got["tri_id"] >= 0:
                            hit, hit_inst, tmax = (got["tri_id"], got["t"], got["u"], got["v"]), inst_id[j] & 0x7FFFFFFF, float(got["t"])
                            if any_hit:
                                done = True
                                break
                        if inst_id[j] < 0:
                            break
                        j += 1
                    if done:
                        break
                    top = mem[ptr]; ptr -= 1
            hits[start + k] = hit
            ids[start + k], peaks[start + k] = hit_inst, peak
    return hits, ids, peaks


def trace(oracle, tlas, inst, nodes, tris, rays, any_hit=False):
    """(hits HIT1, instance ids int32) as hip_traverse_instanced_bvh2_tri1_async writes them; `oracle` is oracle.binding."""
    return _walk(oracle, tlas, inst, nodes, tris, rays, any_hit, False)[:2]


def peak(oracle, tlas, inst, nodes, tris, rays, any_hit=False):
    """Every ray's P: the maximum, over the instances it enters, of (TLAS entries held + the object's deepest stack for the ray)."""
    return _walk(oracle, tlas, inst, nodes, tris, rays, any_hit, True)[2]
