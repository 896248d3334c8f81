"""Deforming meshes under motion (C ABI include/rodent_motion.h): a BVH2 / Tri1 hierarchy whose records hold the mesh at time 0 and at
time 1, traced with a time per ray.

    bvh  = gpubuild.build_bvh2(vertices0, indices)                      # any BVH2 / Tri1 DeviceBvh: the topology
    mbvh = build_motion_bvh2(bvh, vertices0, vertices1, indices)        # both keys refitted over it and fused, on the device
    hits = trace_motion(mbvh, rays, times)                              # one float32 time in [0, 1] per ray
    build_motion_bvh2(bvh, moved0, moved1, indices, out=mbvh)           # the next frame: the same call, in place

A ray whose time is not in [0, 1] (a NaN included) is a miss.  A pre-split tree (build_bvh2(split_budget=...)) can be used as the
topology: the build refits it, which gives every reference its whole triangle's box; `fuse` of two such trees as they come from the
builder is NOT valid, their clipped boxes hold for one key only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi, formats as F
from .gpubuild import INFO_WORDS, BuildError, _ERRORS, ERR_NUM_NODES, _columns4, _enqueue, _mesh, _raise_flags


class MotionBvh:
    """Motion records resident in HBM: `nodes` (num_nodes RodentMotionNode2) and `tris` (num_tris RodentMotionTri1) as uint8 CUDA
    tensors, the info words of the call that made them, the scratch tensor it used (None for `fuse` and `upload`)."""

    def __init__(self, nodes, tris, num_nodes, num_tris, info, scratch=None, dev=0):
        self.nodes, self.tris, self.num_nodes, self.num_tris = nodes, tris, int(num_nodes), int(num_tris)
        self.info, self.scratch, self.dev = info, scratch, dev


def _need_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")


def _records(bvh: abi.DeviceBvh, out, who):
    """The output tensors for the topology `bvh`: new ones, or those of `out` when they have the room."""
    if bvh.width != 2:
        raise ValueError(f"{who}: a BVH2 / Tri1 hierarchy is needed")
    nb, tb = bvh.num_nodes * F.MOTION_NODE2.itemsize, bvh.num_tris * F.MOTION_TRI1.itemsize
    if out is None:
        cuda = f"cuda:{bvh.dev}"
        return torch.empty(nb, dtype=torch.uint8, device=cuda), torch.empty(tb, dtype=torch.uint8, device=cuda)
    if out.nodes.numel() * out.nodes.element_size() < nb or out.tris.numel() * out.tris.element_size() < tb:
        raise ValueError(f"{who}: the buffers of `out` are too small for this hierarchy")
    return out.nodes, out.tris


def _finish(out, nodes, tris, bvh, words, scratch):
    if out is None:
        return MotionBvh(nodes, tris, bvh.num_nodes, bvh.num_tris, words.copy(), scratch, bvh.dev)
    out.num_nodes, out.num_tris, out.info, out.scratch = bvh.num_nodes, bvh.num_tris, words.copy(), scratch
    return out


def build_motion_bvh2(bvh: abi.DeviceBvh, vertices0, vertices1, indices, stream=None, scratch=None, out=None, check=True) -> MotionBvh:
    """The motion records of the topology `bvh` (of gpubuild.build_bvh2, any options, or of any other builder; it is only read) over
    `vertices0` at time 0 and `vertices1` at time 1 (rodent_hip_build_motion_bvh2_tri1).  Arrays and stream as in gpubuild.build_bvh2:
    numpy arrays or CUDA tensors, (n, 3) or (n, 4); `indices` is the triangle table the hierarchy's prim ids refer to.
    scratch / out: reuse the scratch tensor / the record tensors of an earlier result: `out=` is the refit of a motion hierarchy, in
    place.  info: [0] nodes completed at key 0 [1] records fused [2] flags [3] nodes completed at key 1.
    check: raise BuildError on the device's flags and on an incomplete key (default); False returns the result with its info words."""
    _need_gpu()
    nodes, tris = _records(bvh, out, "build_motion_bvh2")
    dev = bvh.dev
    v0, ix, stream = _mesh(vertices0, indices, dev, stream)
    v1 = _columns4(vertices1, torch.float32, dev)
    if v0.shape[0] != v1.shape[0]:
        raise ValueError(f"build_motion_bvh2: {v0.shape[0]} vertices at time 0, {v1.shape[0]} at time 1")
    entry = "rodent_hip_build_motion_bvh2_tri1"
    need = abi.lib().rodent_hip_motion_bvh2_scratch_bytes(bvh.num_nodes, bvh.num_tris)
    if need < 0:
        raise BuildError(f"{entry}: {_ERRORS[ERR_NUM_NODES]}")
    if scratch is None and out is not None:
        scratch = out.scratch
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=f"cuda:{dev}")
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=f"cuda:{dev}")
    words = _enqueue(entry, dev, stream, info, (v0, v1, ix, scratch, bvh.nodes, bvh.tris, nodes, tris), v0.data_ptr(), v1.data_ptr(),
                     v0.shape[0], ix.data_ptr(), ix.shape[0], bvh.nodes.data_ptr(), bvh.num_nodes, bvh.tris.data_ptr(), bvh.num_tris,
                     nodes.data_ptr(), tris.data_ptr(), scratch.data_ptr())
    result = _finish(out, nodes, tris, bvh, words, scratch)
    if check:
        _raise_flags(entry, words)
        if words[0] != bvh.num_nodes or words[3] != bvh.num_nodes:
            raise BuildError(f"{entry}: malformed hierarchy ({words[0]} and {words[3]} of {bvh.num_nodes} nodes completed)")
    return result


def fuse(bvh0: abi.DeviceBvh, bvh1: abi.DeviceBvh, stream=None, out=None, check=True) -> MotionBvh:
    """The motion records of two BVH2 / Tri1 hierarchies of ONE topology, `bvh0` at time 0 and `bvh1` at time 1
    (rodent_hip_fuse_motion_bvh2_tri1): what build_motion_bvh2 ends with.  Both must carry whole-triangle boxes (refitted, or built
    without pre-splitting).  info: [0] 0 [1] records fused [2] flags [3] 0.  Raises BuildError (unless check=False) when the child
    words or the Tri1 w words of the two differ."""
    _need_gpu()
    if bvh1.width != 2 or (bvh0.num_nodes, bvh0.num_tris, bvh0.dev) != (bvh1.num_nodes, bvh1.num_tris, bvh1.dev):
        raise ValueError("fuse: two BVH2 / Tri1 hierarchies with the same record counts on one device are needed")
    nodes, tris = _records(bvh0, out, "fuse")
    dev = bvh0.dev
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=f"cuda:{dev}")
    entry = "rodent_hip_fuse_motion_bvh2_tri1"
    words = _enqueue(entry, dev, stream, info, (bvh0.nodes, bvh0.tris, bvh1.nodes, bvh1.tris, nodes, tris), bvh0.nodes.data_ptr(),
                     bvh0.tris.data_ptr(), bvh1.nodes.data_ptr(), bvh1.tris.data_ptr(), bvh0.num_nodes, bvh0.num_tris, nodes.data_ptr(),
                     tris.data_ptr())
    result = _finish(out, nodes, tris, bvh0, words, None)
    if check:
        _raise_flags(entry, words)
    return result


def upload(motion_nodes: np.ndarray, motion_tris: np.ndarray, dev=0) -> MotionBvh:
    """A MotionBvh of host records (formats.MOTION_NODE2 / MOTION_TRI1), as they are."""
    _need_gpu()
    nodes, tris = np.ascontiguousarray(motion_nodes, F.MOTION_NODE2), np.ascontiguousarray(motion_tris, F.MOTION_TRI1)
    return MotionBvh(abi.to_device(nodes, dev), abi.to_device(tris, dev), len(nodes), len(tris),
                     np.int32([0, len(nodes) + len(tris), 0, 0]), None, dev)


def trace_motion_async(mbvh: MotionBvh, rays_dev, times_dev, hits_dev, num_rays, any_hit=False, stream=None):
    """Enqueues one traversal pass on `stream` (torch stream or None = torch's current stream): `times_dev` holds one float32 per ray.
    A stack overflow is reported by abi.check_errors."""
    if stream is None:
        stream = torch.cuda.current_stream(mbvh.dev)
    abi.lib().hip_traverse_motion_bvh2_tri1_async(mbvh.dev, mbvh.nodes.data_ptr(), mbvh.tris.data_ptr(), rays_dev.data_ptr(),
                                                  times_dev.data_ptr(), hits_dev.data_ptr(), int(num_rays), int(any_hit),
                                                  C.c_void_p(stream.cuda_stream))


def trace_motion(mbvh: MotionBvh, rays: np.ndarray, times, any_hit=False) -> np.ndarray:
    """Synchronous convenience wrapper: host rays and their times (one float32 each) in, host Hit1 array out."""
    _need_gpu()
    dev, n = mbvh.dev, len(rays)
    times = np.ascontiguousarray(times, np.float32)
    if times.shape != (n,):
        raise ValueError(f"trace_motion: expected {n} times, got shape {times.shape}")
    rays_dev = abi.to_device(rays, dev)
    times_dev = torch.from_numpy(times if n else np.zeros(1, np.float32)).to(f"cuda:{dev}")
    hits_dev = torch.zeros(max(n, 1) * F.HIT1.itemsize, dtype=torch.uint8, device=f"cuda:{dev}")
    torch.cuda.synchronize(dev)
    fn = abi.lib().hip_occluded_motion_bvh2_tri1 if any_hit else abi.lib().hip_intersect_motion_bvh2_tri1
    fn(dev, mbvh.nodes.data_ptr(), mbvh.tris.data_ptr(), rays_dev.data_ptr(), times_dev.data_ptr(), hits_dev.data_ptr(), n)
    return abi.from_device(hits_dev, F.HIT1)[:n]


def download(mbvh: MotionBvh):
    """(nodes MOTION_NODE2, tris MOTION_TRI1) host copies of a MotionBvh."""
    nodes = mbvh.nodes.view(torch.uint8)[: mbvh.num_nodes * F.MOTION_NODE2.itemsize].cpu().numpy().view(F.MOTION_NODE2).copy()
    tris = mbvh.tris.view(torch.uint8)[: mbvh.num_tris * F.MOTION_TRI1.itemsize].cpu().numpy().view(F.MOTION_TRI1).copy()
    return nodes, tris
