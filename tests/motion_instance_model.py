"""CPU model of moving instances (the section "moving instances" of include/rodent_instances.h; rodent_amd/csrc/build_tlas.h:
k_motion_instances, traversal_instanced.h: k_instanced_motion) in numpy, on top of tests/instance_model.py, which stays as it is.

  lerp                 the placement at a time: s = 1 - t; m = s * m0 + t * m1, two products and a sum, each rounded to float32
  widening, motion_box the static rule's per-axis widening e, and the box over both endpoint boxes widened by e0 + e1 again
  build_motion_tlas    the motion instance stage, then lbvh_model's morton_codes / karras / emit, as instance_model.build_tlas
  trace / peak         rays grouped by the bits of their time; per group a static INSTANCE array in leaf order from invert(lerp(M0, M1, t))
                       goes to instance_model's walk over the motion TLAS's nodes
A skipped instance is a REAL skip: its stand-in record names no object (node_offset = the end of the node array, so the slice the walk
hands to the oracle is empty), and `_Skipping`, the oracle the walk is given, answers an empty object itself -- no hit, and a depth that
keeps the instance out of the stack peak -- without entering anything.  tmax and the hit stay as they are, the walk goes on to the next
instance of the leaf.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import lbvh_model as L
from rodent_amd import formats as F

F32 = np.float32


def descriptors(transforms0, transforms1, object_ids, instance_ids=None):
    """The MOTION_INSTANCE_DESC array of two sets of (n, 12) / (n, 3, 4) transforms."""
    t0 = np.asarray(transforms0, F32).reshape(len(transforms0), 12)
    d = np.zeros(len(t0), F.MOTION_INSTANCE_DESC)
    d["object_to_world0"], d["object_to_world1"], d["object"] = t0, np.asarray(transforms1, F32).reshape(len(t0), 12), object_ids
    d["instance_id"] = np.arange(len(t0)) if instance_ids is None else instance_ids
    return d


def lerp(m0, m1, t):
    """The placements (n, 12) float32 at time t (a float32, or one per matrix): used as given, never clamped."""
    m0, m1 = np.asarray(m0, F32).reshape(-1, 12), np.asarray(m1, F32).reshape(-1, 12)
    t = np.asarray(t, F32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        s = F32(1) - t
        return (s * m0 + t * m1).astype(F32)


def widening(m, olo, ohi):
    """The static rule's per-axis widening e (n, 3) of object boxes olo / ohi (n, 3) under matrices m (n, 12)."""
    m = np.asarray(m, F32).reshape(-1, 3, 4)
    olo, ohi = np.asarray(olo, F32).reshape(-1, 3), np.asarray(ohi, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        mag = np.fmax(np.abs(olo), np.abs(ohi))
        a = np.abs(m)
        return F32(2.0 ** -21) * (((a[:, :, 0] * mag[:, 0:1] + a[:, :, 1] * mag[:, 1:2]) + a[:, :, 2] * mag[:, 2:3]) + a[:, :, 3])


def motion_box(m0, m1, olo, ohi):
    """The motion boxes (n, 6: lo_x hi_x lo_y hi_y lo_z hi_z): fmin / fmax over the two widened endpoint boxes, moved outward by e0 + e1."""
    b0, b1 = M.world_box(m0, olo, ohi), M.world_box(m1, olo, ohi)
    box = np.empty_like(b0)
    with np.errstate(all="ignore"):
        e = widening(m0, olo, ohi) + widening(m1, olo, ohi)
        box[:, 0::2] = np.fmin(b0[:, 0::2], b1[:, 0::2]) - e
        box[:, 1::2] = np.fmax(b0[:, 1::2], b1[:, 1::2]) + e
    return box


def build_motion_tlas(nodes, table, descs, max_leaf=1):
    """(tlas nodes NODE2, instances MOTION_INSTANCE in leaf order, info int32[4]) as rodent_hip_build_motion_tlas writes them."""
    assert 1 <= max_leaf <= 8 and 1 <= len(descs) <= 1 << 22 and len(table) >= 1
    flags = 0
    obj = descs["object"].astype(np.int64)
    outside = (obj < 0) | (obj >= len(table))
    if outside.any():
        flags |= M.BAD_OBJECT
    ob = table[np.where(outside, 0, obj)]
    m0, m1 = descs["object_to_world0"], descs["object_to_world1"]
    if M.invert(m0)[1].any() or M.invert(m1)[1].any():
        flags |= M.BAD_TRANSFORM
    roots = nodes[ob["node_offset"]]["bounds"]
    olo, ohi = np.fmin(roots[:, 0:6:2], roots[:, 6:12:2]), np.fmax(roots[:, 1:6:2], roots[:, 7:12:2])
    box = motion_box(m0, m1, olo, ohi)
    with np.errstate(all="ignore"):
        points = box[:, 0::2] + box[:, 1::2]
        codes = L.morton_codes(points)
    order = np.lexsort((np.arange(len(codes)), codes))
    t_nodes, marked, info = L.emit(codes[order], box[order], np.zeros(len(order), F.TRI1),
                                   (descs["instance_id"][order] & 0x7FFFFFFF).astype(np.int64), max_leaf)
    inst = np.zeros(len(order), F.MOTION_INSTANCE)
    inst["object_to_world0"], inst["object_to_world1"] = m0[order], m1[order]
    inst["node_offset"], inst["tri_offset"] = ob["node_offset"][order], ob["tri_offset"][order]
    inst["instance_id"] = marked["prim_id"]
    info[2] = flags
    return t_nodes, inst, info


# ---- traversal ------------------------------------------------------------------------------------------------------------------------
def placed(minst, t, num_nodes):
    """(the static INSTANCE array of motion instances `minst` at time t, which of them are skipped): world_to_object =
    invert(lerp(M0, M1, t)); a skipped instance names the empty object at the end of the node array."""
    w, skipped = M.invert(lerp(minst["object_to_world0"], minst["object_to_world1"], t))
    inst = np.zeros(len(minst), F.INSTANCE)
    inst["world_to_object"] = w
    inst["node_offset"], inst["tri_offset"] = np.where(skipped, num_nodes, minst["node_offset"]), minst["tri_offset"]
    inst["instance_id"] = minst["instance_id"]
    return inst, skipped


class _Skipping:
    """oracle.binding for instance_model's walk, with the empty object answered here: not entered, no hit, no stack."""

    def __init__(self, oracle):
        self.oracle = oracle

    def traverse(self, width, nodes, tris, ray, any_hit=False):
        if len(nodes) == 0:
            return np.array([(-1, 0, 0, 0)], F.HIT1), None
        return self.oracle.traverse(width, nodes, tris, ray, any_hit=any_hit)

    def ray_depths(self, nodes, tris, ray, any_hit=False):
        if len(nodes) == 0:
            return [-(1 << 30)]                                          # max(peak, held + this) keeps the peak
        return self.oracle.ray_depths(nodes, tris, ray, any_hit=any_hit)


def time_groups(times):
    """[(time, ray indices)] per distinct bit pattern of the times."""
    bits = np.ascontiguousarray(times, F32).view("<u4")
    return [(np.array([b], "<u4").view(F32)[0], np.flatnonzero(bits == b)) for b in np.unique(bits)]


def _walk(oracle, tlas, minst, nodes, tris, rays, times, any_hit, want_peak):
    assert len(times) == len(rays)
    hits, ids, peaks = np.zeros(len(rays), F.HIT1), np.full(len(rays), -1, np.int32), np.zeros(len(rays), np.int64)
    for t, sel in time_groups(times):
        inst, _ = placed(minst, t, len(nodes))
        h, i, p = M._walk(_Skipping(oracle), tlas, inst, nodes, tris, rays[sel], any_hit, want_peak)
        hits[sel], ids[sel], peaks[sel] = h, i, p
    return hits, ids, peaks


def trace(oracle, tlas, minst, nodes, tris, rays, times, any_hit=False):
    """(hits HIT1, instance ids int32) as hip_traverse_motion_instanced_bvh2_tri1_async writes them; `oracle` is oracle.binding."""
    return _walk(oracle, tlas, minst, nodes, tris, rays, times, any_hit, False)[:2]


def peak(oracle, tlas, minst, nodes, tris, rays, times, any_hit=False):
    """Every ray's P at its own time (instance_model.peak; a skipped instance holds nothing)."""
    return _walk(oracle, tlas, minst, nodes, tris, rays, times, any_hit, True)[2]
