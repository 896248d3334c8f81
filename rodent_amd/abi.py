"""ctypes binding of librodent_hip.so (the C ABI declared in include/rodent_traversal.h).

This is the Python-side mirror of what the reference's bench_traversal.cpp does
with the AnyDSL-generated traversal.h: hand device pointers to the entry points.
Device memory comes from torch (plumbing only); every entry point receives raw
pointers.  There is NO CPU fallback: if the shared library is missing or no GPU is
visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
# torch before the library, always: torch's bundled HIP runtime (torch/lib/libamdhip64.so) carries the soname the library links
# (libamdhip64.so.7), so once torch is loaded the library binds to that same runtime.  Loaded the other way round, the library pulls in
# the system ROCm runtime and torch then maps its own beside it: two HIP runtimes on one device (torch sees no GPU, or launches abort).
import torch  # noqa: F401

from . import formats as F

# RODENT_HIP_LAB=1 selects the lab build (librodent_hip_lab.so: the product kernels plus every measured-and-lost variant
# and the instrumented builds; made by `RODENT_HIP_LAB=1 python -m rodent_amd.build`).  Default: the product library.
LAB = os.environ.get("RODENT_HIP_LAB", "0") not in ("", "0")
LIB_PATH = Path(__file__).resolve().parent / "lib" / ("librodent_hip_lab.so" if LAB else "librodent_hip.so")
# lab: another build of the library (A/B runs of compiler options, scripts/flags_experiment.sh)
if os.environ.get("RODENT_HIP_LIB"):
    LIB_PATH = Path(os.environ["RODENT_HIP_LIB"]).resolve()

SYNC_ENTRY_POINTS = [
    "amdgpu_intersect_single_ray1_bvh2_tri1", "amdgpu_occluded_single_ray1_bvh2_tri1",
    "hip_intersect_single_ray1_bvh4_tri4", "hip_occluded_single_ray1_bvh4_tri4",
    "hip_intersect_single_ray1_bvh8_tri4", "hip_occluded_single_ray1_bvh8_tri4",
]
ASYNC_ENTRY_POINTS = ["hip_traverse_bvh2_tri1_async", "hip_traverse_bvh4_tri4_async", "hip_traverse_bvh8_tri4_async"]
EXPORTS = SYNC_ENTRY_POINTS + ASYNC_ENTRY_POINTS + [
    "rodent_hip_check_errors", "rodent_hip_get_kernel_time", "rodent_hip_device_count", "rodent_hip_num_variants",
        "rodent_hip_variant_name",
    "rodent_hip_kernel_name", "rodent_hip_version", "rodent_hip_source_digest", "rodent_hip_is_lab_build", "rodent_hip_phased_min_rays",
        "rodent_hip_top_min_rays", "rodent_hip_ray_kind_hint", "rodent_hip_ray_grid", "rodent_hip_octant_loops", "rodent_hip_schedule_history",
        "rodent_hip_record_offsets", "rodent_hip_record_offsets_ok",
        "rodent_hip_read_stats", "rodent_hip_read_trace", "rodent_hip_debug_set_perm",
    "rodent_hip_build_scratch_bytes", "rodent_hip_build_bvh2_tri1", "rodent_hip_build_bvh2_tri1_sync",
    "rodent_hip_build_opt_scratch_bytes", "rodent_hip_build_bvh2_tri1_opt", "rodent_hip_build_bvh2_tri1_opt_sync",
    "rodent_hip_build_split_max_refs", "rodent_hip_build_split_scratch_bytes", "rodent_hip_build_bvh2_tri1_split",
    "rodent_hip_build_bvh2_tri1_split_sync",
    "rodent_hip_build_ploc_scratch_bytes", "rodent_hip_build_bvh2_tri1_ploc", "rodent_hip_build_bvh2_tri1_ploc_sync",
    "rodent_hip_refit_scratch_bytes", "rodent_hip_refit_bvh2_tri1", "rodent_hip_refit_bvh2_tri1_sync",
    "rodent_hip_refit_wide_scratch_bytes", "rodent_hip_refit_bvh4_tri4", "rodent_hip_refit_bvh4_tri4_sync",
    "rodent_hip_refit_bvh8_tri4", "rodent_hip_refit_bvh8_tri4_sync",
    "rodent_hip_collapse_scratch_bytes", "rodent_hip_collapse_bvh2_tri1", "rodent_hip_collapse_bvh2_tri1_sync",
    "rodent_hip_collapse_bounded_scratch_bytes", "rodent_hip_collapse_bvh2_tri1_bounded", "rodent_hip_collapse_bvh2_tri1_bounded_sync",
    "rodent_hip_tlas_scratch_bytes", "rodent_hip_build_tlas", "rodent_hip_build_tlas_sync",
    "hip_traverse_instanced_bvh2_tri1_async", "hip_intersect_instanced_bvh2_tri1", "hip_occluded_instanced_bvh2_tri1",
    "rodent_hip_motion_tlas_scratch_bytes", "rodent_hip_build_motion_tlas", "rodent_hip_build_motion_tlas_sync",
    "hip_traverse_motion_instanced_bvh2_tri1_async", "hip_intersect_motion_instanced_bvh2_tri1",
    "hip_occluded_motion_instanced_bvh2_tri1",
    "rodent_hip_refit_objects_plan", "rodent_hip_refit_objects",
    "rodent_hip_build_objects_plan", "rodent_hip_build_objects", "rodent_hip_build_objects_sync",
    "rodent_hip_fuse_motion_bvh2_tri1", "rodent_hip_motion_bvh2_scratch_bytes", "rodent_hip_build_motion_bvh2_tri1",
    "rodent_hip_build_motion_bvh2_tri1_sync",
    "hip_traverse_motion_bvh2_tri1_async", "hip_intersect_motion_bvh2_tri1", "hip_occluded_motion_bvh2_tri1",
    "rodent_hip_motion_objects_scratch_bytes", "rodent_hip_build_motion_objects", "rodent_hip_build_motion_objects_sync",
    "rodent_hip_build_motion_tlas_motion_objects", "rodent_hip_build_motion_tlas_motion_objects_sync",
    "hip_traverse_motion_instanced_motion_bvh2_tri1_async", "hip_intersect_motion_instanced_motion_bvh2_tri1",
    "hip_occluded_motion_instanced_motion_bvh2_tri1",
]
BLOCK_OF_WIDTH = {2: F.BVH2_TRI1, 4: F.BVH4_TRI4, 8: F.BVH8_TRI4}

_lib = None


class BuildOptions(C.Structure):
    """struct RodentBuildOptions (include/rodent_build.h)."""
    _fields_ = [("max_leaf", C.c_int32), ("treelet_passes", C.c_int32), ("node_cost", C.c_float), ("tri_cost", C.c_float)]


class SplitOptions(C.Structure):
    """struct RodentSplitOptions (include/rodent_build.h)."""
    _fields_ = [("budget", C.c_float), ("max_pieces", C.c_int32)]


class PlocOptions(C.Structure):
    """struct RodentPlocOptions (include/rodent_build.h)."""
    _fields_ = [("radius", C.c_int32), ("depth_limit", C.c_int32), ("wide_iterations", C.c_int32)]


class MissingExtension(RuntimeError):
    pass


def lib():
    """Loads librodent_hip.so (built in-tree by rodent_amd.build); raises if absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise MissingExtension(f"{LIB_PATH} not built: run `python -m rodent_amd.build` (needs hipcc)")
        l = C.CDLL(str(LIB_PATH))
        vp, i32 = C.c_void_p, C.c_int32
        for name in SYNC_ENTRY_POINTS:
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, i32]
        for name in ASYNC_ENTRY_POINTS:
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp]
        l.rodent_hip_check_errors.restype = i32; l.rodent_hip_check_errors.argtypes = [i32, vp]
        l.rodent_hip_is_lab_build.restype = i32; l.rodent_hip_is_lab_build.argtypes = []
        l.rodent_hip_phased_min_rays.restype = None; l.rodent_hip_phased_min_rays.argtypes = [i32]
        l.rodent_hip_top_min_rays.restype = None; l.rodent_hip_top_min_rays.argtypes = [i32]
        l.rodent_hip_get_kernel_time.restype = C.c_uint64; l.rodent_hip_get_kernel_time.argtypes = []
        l.rodent_hip_ray_kind_hint.restype = None; l.rodent_hip_ray_kind_hint.argtypes = [i32]
        l.rodent_hip_ray_grid.restype = None; l.rodent_hip_ray_grid.argtypes = [i32]
        l.rodent_hip_octant_loops.restype = None; l.rodent_hip_octant_loops.argtypes = [i32]
        l.rodent_hip_record_offsets.restype = None; l.rodent_hip_record_offsets.argtypes = [i32]
        l.rodent_hip_record_offsets_ok.restype = i32; l.rodent_hip_record_offsets_ok.argtypes = [C.c_uint64] * 4
        l.rodent_hip_schedule_history.restype = None; l.rodent_hip_schedule_history.argtypes = [i32]
        l.rodent_hip_device_count.restype = i32; l.rodent_hip_device_count.argtypes = []
        l.rodent_hip_num_variants.restype = i32; l.rodent_hip_num_variants.argtypes = [i32]
        l.rodent_hip_variant_name.restype = C.c_char_p; l.rodent_hip_variant_name.argtypes = [i32, i32]
        l.rodent_hip_kernel_name.restype = C.c_char_p; l.rodent_hip_kernel_name.argtypes = [i32, i32, i32]
        l.rodent_hip_version.restype = C.c_char_p; l.rodent_hip_version.argtypes = []
        l.rodent_hip_source_digest.restype = C.c_char_p; l.rodent_hip_source_digest.argtypes = []
        l.rodent_hip_read_trace.restype = None; l.rodent_hip_read_trace.argtypes = [i32, C.c_void_p]
        l.rodent_hip_debug_set_perm.restype = None; l.rodent_hip_debug_set_perm.argtypes = [i32, C.c_void_p]
        l.rodent_hip_read_stats.restype = None; l.rodent_hip_read_stats.argtypes = [i32, C.POINTER(C.c_uint64)]
        # device BVH builder (include/rodent_build.h)
        l.rodent_hip_build_scratch_bytes.restype = C.c_int64; l.rodent_hip_build_scratch_bytes.argtypes = [i32]
        l.rodent_hip_build_bvh2_tri1.restype = i32
        l.rodent_hip_build_bvh2_tri1.argtypes = [i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_build_bvh2_tri1_sync.restype = i32
        l.rodent_hip_build_bvh2_tri1_sync.argtypes = [i32, vp, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]
        opt = C.POINTER(BuildOptions)
        l.rodent_hip_build_opt_scratch_bytes.restype = C.c_int64; l.rodent_hip_build_opt_scratch_bytes.argtypes = [i32, opt]
        l.rodent_hip_build_bvh2_tri1_opt.restype = i32
        l.rodent_hip_build_bvh2_tri1_opt.argtypes = [i32, vp, i32, vp, i32, opt, vp, vp, vp, vp, vp]
        l.rodent_hip_build_bvh2_tri1_opt_sync.restype = i32
        l.rodent_hip_build_bvh2_tri1_opt_sync.argtypes = [i32, vp, i32, vp, i32, opt, vp, vp, C.POINTER(i32)]
        spl = C.POINTER(SplitOptions)
        l.rodent_hip_build_split_max_refs.restype = C.c_int64; l.rodent_hip_build_split_max_refs.argtypes = [i32, spl]
        l.rodent_hip_build_split_scratch_bytes.restype = C.c_int64
        l.rodent_hip_build_split_scratch_bytes.argtypes = [i32, opt, spl]
        l.rodent_hip_build_bvh2_tri1_split.restype = i32
        l.rodent_hip_build_bvh2_tri1_split.argtypes = [i32, vp, i32, vp, i32, opt, spl, vp, vp, vp, vp, vp]
        l.rodent_hip_build_bvh2_tri1_split_sync.restype = i32
        l.rodent_hip_build_bvh2_tri1_split_sync.argtypes = [i32, vp, i32, vp, i32, opt, spl, vp, vp, C.POINTER(i32)]
        plo = C.POINTER(PlocOptions)
        l.rodent_hip_build_ploc_scratch_bytes.restype = C.c_int64
        l.rodent_hip_build_ploc_scratch_bytes.argtypes = [i32, opt, spl, plo]
        l.rodent_hip_build_bvh2_tri1_ploc.restype = i32
        l.rodent_hip_build_bvh2_tri1_ploc.argtypes = [i32, vp, i32, vp, i32, opt, spl, plo, vp, vp, vp, vp, vp]
        l.rodent_hip_build_bvh2_tri1_ploc_sync.restype = i32
        l.rodent_hip_build_bvh2_tri1_ploc_sync.argtypes = [i32, vp, i32, vp, i32, opt, spl, plo, vp, vp, C.POINTER(i32)]
        l.rodent_hip_refit_scratch_bytes.restype = C.c_int64; l.rodent_hip_refit_scratch_bytes.argtypes = [i32, i32]
        l.rodent_hip_refit_bvh2_tri1.restype = i32
        l.rodent_hip_refit_bvh2_tri1.argtypes = [i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp]
        l.rodent_hip_refit_bvh2_tri1_sync.restype = i32
        l.rodent_hip_refit_bvh2_tri1_sync.argtypes = [i32, vp, i32, vp, i32, vp, i32, vp, i32, C.POINTER(i32)]
        l.rodent_hip_refit_wide_scratch_bytes.restype = C.c_int64; l.rodent_hip_refit_wide_scratch_bytes.argtypes = [i32, i32, i32]
        for name in ("rodent_hip_refit_bvh4_tri4", "rodent_hip_refit_bvh8_tri4"):
            fn = getattr(l, name); fn.restype = i32; fn.argtypes = l.rodent_hip_refit_bvh2_tri1.argtypes
            fn = getattr(l, name + "_sync"); fn.restype = i32; fn.argtypes = l.rodent_hip_refit_bvh2_tri1_sync.argtypes
        l.rodent_hip_collapse_scratch_bytes.restype = C.c_int64; l.rodent_hip_collapse_scratch_bytes.argtypes = [i32, i32, i32]
        l.rodent_hip_collapse_bvh2_tri1.restype = i32
        l.rodent_hip_collapse_bvh2_tri1.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_collapse_bvh2_tri1_sync.restype = i32
        l.rodent_hip_collapse_bvh2_tri1_sync.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, C.POINTER(i32)]
        l.rodent_hip_collapse_bounded_scratch_bytes.restype = C.c_int64
        l.rodent_hip_collapse_bounded_scratch_bytes.argtypes = [i32, i32, i32]
        l.rodent_hip_collapse_bvh2_tri1_bounded.restype = i32
        l.rodent_hip_collapse_bvh2_tri1_bounded.argtypes = [i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_collapse_bvh2_tri1_bounded_sync.restype = i32
        l.rodent_hip_collapse_bvh2_tri1_bounded_sync.argtypes = [i32, i32, i32, vp, i32, vp, i32, vp, vp, C.POINTER(i32)]
        # instanced scenes (include/rodent_instances.h)
        l.rodent_hip_tlas_scratch_bytes.restype = C.c_int64; l.rodent_hip_tlas_scratch_bytes.argtypes = [i32]
        l.rodent_hip_build_tlas.restype = i32
        l.rodent_hip_build_tlas.argtypes = [i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_build_tlas_sync.restype = i32
        l.rodent_hip_build_tlas_sync.argtypes = [i32, vp, vp, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]
        l.hip_traverse_instanced_bvh2_tri1_async.restype = None
        l.hip_traverse_instanced_bvh2_tri1_async.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
        for name in ("hip_intersect_instanced_bvh2_tri1", "hip_occluded_instanced_bvh2_tri1"):
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, i32]
        # moving instances: the static entries' shapes, `times` behind `rays`
        l.rodent_hip_motion_tlas_scratch_bytes.restype = C.c_int64; l.rodent_hip_motion_tlas_scratch_bytes.argtypes = [i32]
        l.rodent_hip_build_motion_tlas.restype = i32
        l.rodent_hip_build_motion_tlas.argtypes = [i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_build_motion_tlas_sync.restype = i32
        l.rodent_hip_build_motion_tlas_sync.argtypes = [i32, vp, vp, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]
        l.hip_traverse_motion_instanced_bvh2_tri1_async.restype = None
        l.hip_traverse_motion_instanced_bvh2_tri1_async.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
        for name in ("hip_intersect_motion_instanced_bvh2_tri1", "hip_occluded_motion_instanced_bvh2_tri1"):
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32]
        l.rodent_hip_refit_objects_plan.restype = C.c_int64
        l.rodent_hip_refit_objects_plan.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp]
        l.rodent_hip_refit_objects.restype = i32
        l.rodent_hip_refit_objects.argtypes = [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp]
        l.rodent_hip_build_objects_plan.restype = C.c_int64
        l.rodent_hip_build_objects_plan.argtypes = [vp, vp, vp, i32, vp, vp]
        l.rodent_hip_build_objects.restype = i32
        l.rodent_hip_build_objects.argtypes = [i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
        l.rodent_hip_build_objects_sync.restype = i32
        l.rodent_hip_build_objects_sync.argtypes = [i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, i32, vp, vp]
        # deforming meshes under motion (include/rodent_motion.h)
        l.rodent_hip_fuse_motion_bvh2_tri1.restype = i32
        l.rodent_hip_fuse_motion_bvh2_tri1.argtypes = [i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
        l.rodent_hip_motion_bvh2_scratch_bytes.restype = C.c_int64; l.rodent_hip_motion_bvh2_scratch_bytes.argtypes = [i32, i32]
        l.rodent_hip_build_motion_bvh2_tri1.restype = i32
        l.rodent_hip_build_motion_bvh2_tri1.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
        l.rodent_hip_build_motion_bvh2_tri1_sync.restype = i32
        l.rodent_hip_build_motion_bvh2_tri1_sync.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, C.POINTER(i32)]
        l.hip_traverse_motion_bvh2_tri1_async.restype = None
        l.hip_traverse_motion_bvh2_tri1_async.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, vp]
        for name in ("hip_intersect_motion_bvh2_tri1", "hip_occluded_motion_bvh2_tri1"):
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, vp, i32]
        # deforming objects under moving instances (include/rodent_instances.h)
        l.rodent_hip_motion_objects_scratch_bytes.restype = C.c_int64
        l.rodent_hip_motion_objects_scratch_bytes.argtypes = [i32, i32, C.c_int64]
        l.rodent_hip_build_motion_objects.restype = i32
        l.rodent_hip_build_motion_objects.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp,
                                                      vp, vp]
        l.rodent_hip_build_motion_objects_sync.restype = i32
        l.rodent_hip_build_motion_objects_sync.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, vp, vp,
                                                           C.POINTER(i32)]
        l.rodent_hip_build_motion_tlas_motion_objects.restype = i32
        l.rodent_hip_build_motion_tlas_motion_objects.argtypes = l.rodent_hip_build_motion_tlas.argtypes
        l.rodent_hip_build_motion_tlas_motion_objects_sync.restype = i32
        l.rodent_hip_build_motion_tlas_motion_objects_sync.argtypes = l.rodent_hip_build_motion_tlas_sync.argtypes
        l.hip_traverse_motion_instanced_motion_bvh2_tri1_async.restype = None
        l.hip_traverse_motion_instanced_motion_bvh2_tri1_async.argtypes = l.hip_traverse_motion_instanced_bvh2_tri1_async.argtypes
        for name in ("hip_intersect_motion_instanced_motion_bvh2_tri1", "hip_occluded_motion_instanced_motion_bvh2_tri1"):
            fn = getattr(l, name); fn.restype = None; fn.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32]
        _lib = l
    return _lib


def built_from_these_sources() -> bool:
    """Whether the loaded library was compiled from the sources in this tree (its compiled-in digest against build.source_digest())."""
    from . import build
    return lib().rodent_hip_source_digest().decode() == build.source_digest()


def variants(width):
    l = lib()
    return [l.rodent_hip_variant_name(width, i).decode() for i in range(l.rodent_hip_num_variants(width))]


# Mappings that do NOT keep the reference's per-ray visit order (lab build only: work stealing inside the wave, measured and lost): last-bit
# ties in t resolve to another triangle.  Every shipped mapping reproduces the reference kernel bit for bit (tests/). (round 6: deferred
# leaves / triangle turns with deferral visit a superset of the nodes)
ORDER_CHANGING = ("steal", "defer-", "stats-defer", "turns-p")


def order_preserving_variants(width):
    """Indices of the mappings whose hit records equal the reference kernel's bit for bit."""
    return [i for i, n in enumerate(variants(width)) if not n.startswith(ORDER_CHANGING)]


def kernel_name(width, variant, any_hit=False):
    return lib().rodent_hip_kernel_name(width, variant, int(any_hit)).decode()


# ---- device buffers (torch is plumbing: allocation + copies) ---------------------------------

def to_device(arr: np.ndarray, dev: int = 0):
    """Structured numpy array -> torch uint8 CUDA tensor holding the same bytes."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    a = np.ascontiguousarray(arr)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(0, np.uint8))
    return t.to(f"cuda:{dev}")


def from_device(t, dtype: np.dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype).copy()


class DeviceBvh:
    """A BVH resident in HBM: nodes + tris of one layout (2 = Node2/Tri1, 4 = Node4/Tri4, 8 = Node8/Tri4).

    Both arrays lie in ONE allocation (`buffer`; `nodes` and `tris` are views of it, the triangles 256-byte aligned behind the nodes): the
    default BVH2 kernel addresses its records as one base + 32-bit offsets where the two arrays lie within 4 GiB of each other
    (rodent_hip_record_offsets), and two allocations of the same process may lie tens of GiB apart -- measured: 64 ... 220 MiB in plain
    runs, 32.6 GiB in three of four runs under a profiler's kernel trace, where the launches then built 64-bit addresses."""

    def __init__(self, width, nodes, tris, dev=0):
        import torch
        assert width in (2, 4, 8)
        self.width, self.dev = width, dev
        self.num_nodes, self.num_tris = len(nodes), len(tris)
        if not torch.cuda.is_available():
            raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
        nb, tb = (np.ascontiguousarray(a).view(np.uint8).reshape(-1) if len(a) else np.zeros(0, np.uint8) for a in (nodes, tris))
        start = (len(nb) + 255) // 256 * 256
        host = np.zeros(start + len(tb), np.uint8)
        host[:len(nb)] = nb
        host[start:] = tb
        self.buffer = torch.from_numpy(host).to(f"cuda:{dev}")
        self.nodes, self.tris = self.buffer[:len(nb)], self.buffer[start:]

    @classmethod
    def from_tensors(cls, width, nodes, tris, num_nodes, num_tris, dev=0):
        """A BVH that is already on the device: `nodes` and `tris` are CUDA tensors (any dtype) holding at least num_nodes / num_tris
        records of the layout; they are used as they are, not copied."""
        assert width in (2, 4, 8)
        node_dt, tri_dt = {2: (F.NODE2, F.TRI1), 4: (F.NODE4, F.TRI4), 8: (F.NODE8, F.TRI4)}[width]
        for t, count, dt in ((nodes, num_nodes, node_dt), (tris, num_tris, tri_dt)):
            if not t.is_cuda or t.numel() * t.element_size() < count * dt.itemsize or not t.is_contiguous():
                raise ValueError("DeviceBvh.from_tensors: a contiguous CUDA tensor with room for every record is needed")
        self = cls.__new__(cls)
        self.width, self.dev = width, dev
        self.num_nodes, self.num_tris = int(num_nodes), int(num_tris)
        self.nodes, self.tris = nodes, tris
        return self

    @classmethod
    def load(cls, path, width, dev=0):
        nodes, tris = F.read_bvh(path, BLOCK_OF_WIDTH[width])
        return cls(width, nodes, tris, dev)


def traverse_async(bvh: DeviceBvh, rays_dev, hits_dev, num_rays, any_hit=False, variant=0, stream=None):
    """Enqueues one traversal pass on `stream` (torch stream or None = torch's current stream)."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(bvh.dev)
    fn = getattr(lib(), {2: "hip_traverse_bvh2_tri1_async", 4: "hip_traverse_bvh4_tri4_async",
        8: "hip_traverse_bvh8_tri4_async"}[bvh.width])
    fn(bvh.dev, bvh.nodes.data_ptr(), bvh.tris.data_ptr(), rays_dev.data_ptr(), hits_dev.data_ptr(),
       int(num_rays), int(any_hit), int(variant), C.c_void_p(stream.cuda_stream))


def traverse(bvh: DeviceBvh, rays: np.ndarray, any_hit=False, variant=None) -> np.ndarray:
    """Synchronous convenience wrapper: host rays in, host Hit1 array out.

    With variant=None it goes through the reference-named synchronous entry points
    (amdgpu_intersect_single_ray1_bvh2_tri1 & co)."""
    import torch
    n = len(rays)
    rays_dev = to_device(rays, bvh.dev)
    hits_dev = torch.zeros(max(n, 1) * F.HIT1.itemsize, dtype=torch.uint8, device=f"cuda:{bvh.dev}")
    if variant is None:
        torch.cuda.synchronize(bvh.dev)
        name = {(2, False): "amdgpu_intersect_single_ray1_bvh2_tri1", (2, True): "amdgpu_occluded_single_ray1_bvh2_tri1",
                (4, False): "hip_intersect_single_ray1_bvh4_tri4", (4, True): "hip_occluded_single_ray1_bvh4_tri4",
                (8, False): "hip_intersect_single_ray1_bvh8_tri4",
                    (8, True): "hip_occluded_single_ray1_bvh8_tri4"}[(bvh.width, bool(any_hit))]
        getattr(lib(), name)(bvh.dev, bvh.nodes.data_ptr(), bvh.tris.data_ptr(), rays_dev.data_ptr(), hits_dev.data_ptr(), n)
    else:
        traverse_async(bvh, rays_dev, hits_dev, n, any_hit, variant)
        torch.cuda.synchronize(bvh.dev)
        check_errors(bvh.dev)
    return from_device(hits_dev, F.HIT1)[:n]


def schedule_history(enable: bool):
    """rodent_hip_schedule_history: the default BVH2 mapping traces its chunks longest-first by the per-chunk cost the previous
    launch of the same size recorded (off by default; per (device, stream); hit records do not depend on it)."""
    lib().rodent_hip_schedule_history(int(bool(enable)))


def top_min_rays(rays: int):
    """rodent_hip_top_min_rays: launches of fewer rays take the one-chunk kernel instead of the persistent LDS-image kernel
    (< 0: the shipped threshold, 0: every launch through the LDS-image kernel)."""
    lib().rodent_hip_top_min_rays(int(rays))


def ray_kind_hint(enable: bool):
    """rodent_hip_ray_kind_hint: may the default BVH2 mapping remember that a ray list (pointer, count) was incoherent and trace it with
    the refill kernel from its second launch on (default: no -- kernel selection is stateless; hit records do not depend on it)."""
    lib().rodent_hip_ray_kind_hint(int(bool(enable)))


def ray_grid(width: int = -1):
    """rodent_hip_ray_grid: -1 = the default BVH2 kernel recognises camera rays in image order and traces them as 8 x 8-pixel tiles
    (default), 0 = never, > 0 = that image width on trust (hit records do not depend on it)."""
    lib().rodent_hip_ray_grid(int(width))


def octant_loops(enable: bool = True):
    """rodent_hip_octant_loops: may the default BVH2 kernel trace a chunk whose rays share their direction signs with the loop compiled for
    that octant (default: yes; hit records do not depend on it; read_stats()[3] counts workgroup 0's chunks that took such a loop)."""
    lib().rodent_hip_octant_loops(int(bool(enable)))


def record_offsets(enable: bool = True):
    """rodent_hip_record_offsets: may the default BVH2 kernel address its node and triangle records as one scalar base + a 32-bit byte
    offset per lane where the two arrays lie close enough (default: yes; hit records do not depend on it; read_stats()[1] counts the
    launches that did, read_stats()[0] those that built 64-bit addresses)."""
    lib().rodent_hip_record_offsets(int(bool(enable)))


def record_offsets_ok(nodes: int, node_bytes: int, tris: int, tri_bytes: int) -> bool:
    """rodent_hip_record_offsets_ok: the launch-time predicate on plain integers -- the two pointer values and the bytes mapped from each
    pointer on (needs no GPU)."""
    return bool(lib().rodent_hip_record_offsets_ok(int(nodes), int(node_bytes), int(tris), int(tri_bytes)))


def check_errors(dev=0, stream=None):
    """The asynchronous entry points report a traversal-stack overflow (more than the reference's 64 entries,
    stack.impala:53) through a device-side flag: this waits for `stream`, reads and clears it, and raises."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    if lib().rodent_hip_check_errors(dev, C.c_void_p(stream.cuda_stream)):
        raise RuntimeError("rodent_hip: traversal stack overflow (more than 64 entries)")


def read_stats(dev=0):
    """Phase counters of the instrumented "stats-*" variants (reads and clears)."""
    buf = (C.c_uint64 * 8)()
    lib().rodent_hip_read_stats(dev, buf)
    return list(buf)


def read_trace(dev=0, arm_only=False):
    """Per-wave timeline of the instrumented variants: array [16384, 4] of uint64 (see the header)."""
    if arm_only:
        lib().rodent_hip_read_trace(dev, None)
        return None
    buf = np.zeros((16384, 4), np.uint64)
    lib().rodent_hip_read_trace(dev, buf.ctypes.data_as(C.c_void_p))
    return buf
