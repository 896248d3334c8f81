"""CPU model of deforming meshes under motion (include/rodent_motion.h; rodent_amd/csrc/build_motion.h: k_fuse_motion,
traversal_motion.h: k_bvh2_motion) in numpy, on top of tests/refit_model.py, which stays as it is.

  fuse          two same-topology hierarchies -> MOTION_NODE2 / MOTION_TRI1 with the bounds widened by 2^-19 * M, and the info words
  build         refit_model.refit at both keys, then fuse: the bytes and info words of rodent_hip_build_motion_bvh2_tri1
  lerp          a value at a time: s = 1 - t; x = s * x0 + t * x1, two products and a sum, each rounded to float32
  at_time       the static NODE2 / TRI1 hierarchy the kernel sees at time t (an empty slot keeps its stored (+inf, -inf))
  traced        the time rule: which rays are traced at all
  trace / peak  rays grouped by the bits of their time (motion_instance_model.time_groups); per group at_time goes to the oracle
"""
from __future__ import annotations

import numpy as np

import refit_model as R
from motion_instance_model import time_groups
from rodent_amd import formats as F

F32 = np.float32
BAD_TOPOLOGY = R.BAD_TOPOLOGY
WIDEN = F32(2.0 ** -19)
GEOMETRY = ("v0", "e1", "e2")
WORDS = ("pad", "geom_id", "prim_id")


def fuse(nodes0, tris0, nodes1, tris1, widen=WIDEN):
    """(motion nodes MOTION_NODE2, motion tris MOTION_TRI1, info int32[4]) as rodent_hip_fuse_motion_bvh2_tri1 writes them:
    info = [0, records fused, flags, 0].  `widen`: the constant of the rule (the tests also run it with 0)."""
    assert len(nodes0) == len(nodes1) and len(tris0) == len(tris1)
    mn, mt = np.zeros(len(nodes0), F.MOTION_NODE2), np.zeros(len(tris0), F.MOTION_TRI1)
    flags = 0
    if not np.array_equal(nodes0["child"], nodes1["child"]):
        flags |= BAD_TOPOLOGY
    b0, b1 = nodes0["bounds"].copy(), nodes1["bounds"].copy()
    taken = np.repeat(nodes0["child"] != 0, 6, axis=1)                   # (n, 12): the bounds of slots that have a child
    with np.errstate(all="ignore"):
        lo0, hi0, lo1, hi1 = b0[:, 0::2], b0[:, 1::2], b1[:, 0::2], b1[:, 1::2]
        m = np.fmax(np.fmax(np.abs(lo0), np.abs(hi0)), np.fmax(np.abs(lo1), np.abs(hi1)))
        e = (F32(widen) * m).astype(F32)
        w0, w1 = b0.copy(), b1.copy()
        w0[:, 0::2], w0[:, 1::2], w1[:, 0::2], w1[:, 1::2] = lo0 - e, hi0 + e, lo1 - e, hi1 + e
    mn["bounds0"], mn["bounds1"] = np.where(taken, w0, b0), np.where(taken, w1, b1)
    mn["child"] = nodes0["child"]
    mn["pad"][:, :2] = nodes0["pad"]
    mt["key0"] = tris0
    for name in GEOMETRY:
        mt["key1"][name] = tris1[name]
    if any(not np.array_equal(tris0[w], tris1[w]) for w in WORDS):
        flags |= BAD_TOPOLOGY
    return mn, mt, np.int32([0, len(mn) + len(mt), flags, 0])


def build(nodes, tris, vertices0, vertices1, indices, widen=WIDEN):
    """(motion nodes, motion tris, info) as rodent_hip_build_motion_bvh2_tri1 writes them over the topology nodes / tris:
    info = [nodes completed at key 0, records fused, the OR of all flags, nodes completed at key 1]."""
    n0, t0, i0 = R.refit(nodes, tris, vertices0, indices)
    n1, t1, i1 = R.refit(nodes, tris, vertices1, indices)
    mn, mt, info = fuse(n0, t0, n1, t1, widen)
    return mn, mt, np.int32([i0[0], info[1], i0[2] | i1[2] | info[2], i1[0]])


def lerp(x0, x1, t):
    """The values at time t (a float32): s = 1 - t; s * x0 + t * x1 in float32, every operation rounded on its own."""
    t = F32(t)
    with np.errstate(all="ignore"):
        s = F32(1) - t
        return (s * np.asarray(x0, F32) + t * np.asarray(x1, F32)).astype(F32)


def at_time(mn, mt, t):
    """(nodes NODE2, tris TRI1): the hierarchy the kernel walks at time t."""
    nodes, tris = np.zeros(len(mn), F.NODE2), mt["key0"].copy()
    taken = np.repeat(mn["child"] != 0, 6, axis=1)
    nodes["bounds"] = np.where(taken, lerp(mn["bounds0"], mn["bounds1"], t), mn["bounds0"])
    nodes["child"], nodes["pad"] = mn["child"], mn["pad"][:, :2]
    for name in GEOMETRY:
        tris[name] = lerp(mt["key0"][name], mt["key1"][name], t)
    return nodes, tris


def traced(times):
    """The time rule: 0 <= t <= 1; a NaN fails it, -0 and 1 pass."""
    t = np.asarray(times, F32)
    with np.errstate(invalid="ignore"):
        return (t >= 0) & (t <= 1)


def _walk(oracle, mn, mt, rays, times, any_hit, want_peak):
    assert len(times) == len(rays)
    hits, peaks = np.zeros(len(rays), F.HIT1), np.zeros(len(rays), np.int64)
    hits["tri_id"], hits["t"] = -1, rays["tmax"]                         # the miss record of a refused time
    for t, sel in time_groups(times):
        if not traced(t):
            continue
        nodes, tris = at_time(mn, mt, t)
        if want_peak:
            peaks[sel] = oracle.ray_depths(nodes, tris, rays[sel], any_hit=any_hit)
        else:
            hits[sel] = oracle.traverse(2, nodes, tris, rays[sel], any_hit=any_hit)[0]
    return hits, peaks


def trace(oracle, mn, mt, rays, times, any_hit=False):
    """Hit records (HIT1) as hip_traverse_motion_bvh2_tri1_async writes them; `oracle` is oracle.binding."""
    return _walk(oracle, mn, mt, rays, times, any_hit, False)[0]


def peak(oracle, mn, mt, rays, times, any_hit=False):
    """Every traced ray's deepest stack pointer at its own time (oracle.ray_depths; 0 for a refused time)."""
    return _walk(oracle, mn, mt, rays, times, any_hit, True)[1]
