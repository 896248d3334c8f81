"""CPU model of deforming objects under moving instances (the section of that name of include/rodent_instances.h;
rodent_amd/csrc/bvh_build.hip: rodent_hip_build_motion_objects, build_tlas.h: k_motion_instances over motion roots,
traversal_instanced.h: k_instanced_motion_objects) in numpy, on top of tests/motion_bvh_model.py, motion_instance_model.py,
instance_model.py and refit_model.py, which stay as they are.

  build              motion_bvh_model.build per object over its slice of the packed topology: the packed MOTION_NODE2 / MOTION_TRI1
                     arrays and the info words of rodent_hip_build_motion_objects
  object_box         fmin of the lows / fmax of the highs over the root record's four stored child boxes (two slots at both keys)
  build_motion_tlas  motion_instance_model.build_motion_tlas with that box: a NODE2 stand-in array carries it in the root slots, so the
                     motion instance stage, the sort and the emission are that model's, unedited
  trace / peak       rays grouped by the bits of their time (time_groups): a refused time gives the miss record and id -1; otherwise
                     motion_bvh_model.at_time over the PACKED arrays (it is elementwise, child ids stay object-local), then
                     motion_instance_model.placed and instance_model's walk with _Skipping
"""
from __future__ import annotations

import numpy as np

import instance_model as M
import motion_bvh_model as B
import motion_instance_model as MI
from rodent_amd import formats as F

F32 = np.float32


def build(nodes, tris, table, vertices0, vertices1, indices, ranges):
    """(motion nodes MOTION_NODE2, motion tris MOTION_TRI1, info int32[4]) as rodent_hip_build_motion_objects writes them over the packed
    topology nodes / tris (table: OBJECT rows; ranges: one (first_tri, num_tris) row of `indices` per object): info = [nodes completed at
    key 0, records fused, the OR of all flags, nodes completed at key 1].  Records outside every object are fused as they lie."""
    indices = np.asarray(indices, np.int32).reshape(len(indices), -1)
    mn, mt, _ = B.fuse(nodes, tris, nodes, tris)                          # what lies outside every object: both copies as they are
    info = np.int32([0, len(nodes) + len(tris), 0, 0])
    for ob, (first, count) in zip(table, np.asarray(ranges).reshape(-1, 2)):
        ns = slice(int(ob["node_offset"]), int(ob["node_offset"]) + int(ob["num_nodes"]))
        ts = slice(int(ob["tri_offset"]), int(ob["tri_offset"]) + int(ob["num_tris"]))
        mn[ns], mt[ts], i = B.build(nodes[ns], tris[ts], vertices0, vertices1, indices[first: first + count])
        info[0] += i[0]; info[2] |= i[2]; info[3] += i[3]
    return mn, mt, info


def object_box(roots):
    """(olo, ohi) (n, 3) of root records MOTION_NODE2: over the four stored child boxes; an empty slot's (+inf, -inf) drops out."""
    b0, b1 = roots["bounds0"], roots["bounds1"]
    lo = np.fmin(np.fmin(b0[:, 0:6:2], b0[:, 6:12:2]), np.fmin(b1[:, 0:6:2], b1[:, 6:12:2]))
    hi = np.fmax(np.fmax(b0[:, 1:6:2], b0[:, 7:12:2]), np.fmax(b1[:, 1:6:2], b1[:, 7:12:2]))
    return lo, hi


def key0_box(roots):
    """The box a static reading of key 0 would take: NOT the rule (tests/test_motion_objects_model.py shows that it fails)."""
    b0 = roots["bounds0"]
    return np.fmin(b0[:, 0:6:2], b0[:, 6:12:2]), np.fmax(b0[:, 1:6:2], b0[:, 7:12:2])


def _stand_in(mn, table, box=object_box):
    """A NODE2 array whose record at every object's node_offset holds that object's box in slot 0 and an empty slot 1: what
    motion_instance_model.build_motion_tlas reads of the objects."""
    nodes = np.zeros(len(mn), F.NODE2)
    at = table["node_offset"]
    lo, hi = box(mn[at])
    bounds = np.zeros((len(at), 12), F32)
    bounds[:, 0:6:2], bounds[:, 1:6:2] = lo, hi
    bounds[:, 6:12:2], bounds[:, 7:12:2] = np.inf, -np.inf
    nodes["bounds"][at] = bounds
    return nodes


def build_motion_tlas(mn, table, descs, max_leaf=1, box=object_box):
    """(tlas nodes NODE2, instances MOTION_INSTANCE in leaf order, info int32[4]) as rodent_hip_build_motion_tlas_motion_objects writes
    them."""
    return MI.build_motion_tlas(_stand_in(mn, table, box), table, descs, max_leaf)


def _walk(oracle, tlas, minst, mn, mt, rays, times, any_hit, want_peak):
    assert len(times) == len(rays)
    hits, ids, peaks = np.zeros(len(rays), F.HIT1), np.full(len(rays), -1, np.int32), np.zeros(len(rays), np.int64)
    hits["tri_id"], hits["t"] = -1, rays["tmax"]                         # the miss record of a refused time
    for t, sel in MI.time_groups(times):
        if not B.traced(t):
            continue
        nodes, tris = B.at_time(mn, mt, t)
        inst, _ = MI.placed(minst, t, len(nodes))
        h, i, p = M._walk(MI._Skipping(oracle), tlas, inst, nodes, tris, rays[sel], any_hit, want_peak)
        hits[sel], ids[sel], peaks[sel] = h, i, p
    return hits, ids, peaks


def trace(oracle, tlas, minst, mn, mt, rays, times, any_hit=False):
    """(hits HIT1, instance ids int32) as hip_traverse_motion_instanced_motion_bvh2_tri1_async writes them; `oracle` is oracle.binding."""
    return _walk(oracle, tlas, minst, mn, mt, rays, times, any_hit, False)[:2]


def peak(oracle, tlas, minst, mn, mt, rays, times, any_hit=False):
    """Every traced ray's P at its own time (instance_model.peak over the hierarchy of that time; 0 for a refused time)."""
    return _walk(oracle, tlas, minst, mn, mt, rays, times, any_hit, True)[2]
