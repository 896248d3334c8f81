"""ctypes binding of the renderer ABI (include/rodent_render.h): scene upload, render(), film access.

Mirrors what src/driver/driver.cpp does around the generated `render()`:
setup_interface -> (clear_pixels) -> render(settings, iter++) ... -> get_pixels."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

i32, vp = C.c_int32, C.c_void_p


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Settings(C.Structure):
    _fields_ = [("eye", Vec3), ("dir", Vec3), ("up", Vec3), ("right", Vec3), ("width", C.c_float), ("height", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [(n, vp) for n in ("vertices", "normals", "face_normals", "indices", "nodes", "tris", "materials", "lights",
        "light_ids")] + \
               [(n, i32) for n in ("num_vertices", "num_tris", "num_nodes", "num_bvh_tris", "num_materials", "num_lights")] + \
               [(n, vp) for n in ("texcoords", "textures", "texels")] + [("num_textures", i32), ("num_texels", C.c_uint32)]


class SceneTables(C.Structure):
    """RodentSceneTables: device pointers and counts of the tables a scene owns."""
    _fields_ = [(n, vp) for n in ("vertices", "normals", "face_normals", "lights", "tri_shade", "top_image", "top_image_large")] + \
               [(n, i32) for n in ("num_vertices", "num_tris", "num_lights", "top_nodes", "top_nodes_large")]


class ObjectRange(C.Structure):
    """RodentObjectRange: the triangle and light range of one object of an instanced scene."""
    _fields_ = [(n, i32) for n in ("first_tri", "num_tris", "first_light", "num_lights")]


class SceneInstances(C.Structure):
    """RodentSceneInstances: device pointers and counts of an instanced scene's tables."""
    _fields_ = [(n, vp) for n in ("tlas_nodes", "instances", "descs", "objects", "slot_of", "bases", "light_owner", "lights",
                                  "object_lights", "ray_slots", "tlas_info")] + \
               [(n, i32) for n in ("num_instances", "num_objects", "num_tlas_nodes", "num_lights", "num_object_lights",
                                   "ray_slot_capacity")]


# rodent_hip_scene_create_instanced's refusals (RODENT_SCENE_ERR_*)
SCENE_ERR_COUNTS, SCENE_ERR_RANGES, SCENE_ERR_LIGHT, SCENE_ERR_OBJECT, SCENE_ERR_NO_LIGHT, SCENE_ERR_OPTIONS, SCENE_ERR_TABLE, \
    SCENE_ERR_DEVICE = range(-20, -28, -1)
SCENE_ERR_NOT_INSTANCED = -28                              # rodent_hip_scene_deform_prepare's own
SCENE_ERR_MOVING_LIGHT, SCENE_ERR_SHUTTER = -29, -30       # rodent_hip_scene_create_motion's own, rodent_hip_render_shutter's
MOTION_DEPTH_BITS, MOTION_DEPTH_MASK = 8, 0xFF             # a moving scene's depth word: depth | ubits << 8
SCENE_ERRORS = {SCENE_ERR_COUNTS: "a missing table, a count below 1, more than 2^22 instances, or a hierarchy in the description",
                SCENE_ERR_RANGES: "the objects' triangle or light ranges do not tile the tables in order",
                SCENE_ERR_LIGHT: "an emissive triangle names a light outside its object's light range",
                SCENE_ERR_OBJECT: "an instance names an object outside the table",
                SCENE_ERR_NO_LIGHT: "no instance places an object that has a light",
                SCENE_ERR_OPTIONS: "invalid build options",
                SCENE_ERR_TABLE: "a vertex, material or texture index outside its table",
                SCENE_ERR_DEVICE: "the device raised a flag while building",
                SCENE_ERR_MOVING_LIGHT: "an instance of an object with lights has two different placements (lights stay static)"}
# rodent_hip_scene_create_deforming's refusals, where their wording differs
DEFORMING_ERRORS = {SCENE_ERR_COUNTS: "a missing table, a count below 1, or a hierarchy in the description",
                    SCENE_ERR_LIGHT: "an emissive triangle without an entry in the light table",
                    SCENE_ERR_TABLE: "a vertex, material, texture or light index outside its table",
                    SCENE_ERR_MOVING_LIGHT: "an emissive triangle's corners differ between the keys (lights stay static)"}


class SceneMotionKeys(C.Structure):
    """RodentSceneMotionKeys: device pointers of a deforming scene's key tables and of its motion build's info words."""
    _fields_ = [(n, vp) for n in ("vertices0", "vertices1", "normals0", "normals1", "info")] + [("num_vertices", i32)]


class SceneMotionInstances(C.Structure):
    """RodentSceneMotionInstances: device pointers and counts of a moving scene's tables."""
    _fields_ = [(n, vp) for n in ("tlas_nodes", "instances", "descs", "objects", "slot_of", "bases", "light_owner", "lights",
                                  "object_lights", "ray_slots", "tlas_info")] + \
               [(n, i32) for n in ("num_instances", "num_objects", "num_tlas_nodes", "num_lights", "num_object_lights",
                                   "ray_slot_capacity")]


def pack_depth_time(depth, ubits):
    """The depth words (int32) of a moving scene's primary stream: depth (0 ... 255) | ubits (23 bits) << 8; bit 31 stays 0."""
    depth, ubits = np.asarray(depth, np.int64), np.asarray(ubits, np.int64)
    if ((depth < 0) | (depth > MOTION_DEPTH_MASK)).any() or ((ubits < 0) | (ubits >= 1 << 23)).any():
        raise ValueError("pack_depth_time: depth must lie in [0, 255] and ubits in [0, 2^23)")
    return (depth | ubits << MOTION_DEPTH_BITS).astype(np.int32)


def unpack_depth_time(words):
    """(depth, ubits) of depth words as pack_depth_time makes them."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return (w & MOTION_DEPTH_MASK).astype(np.int32), (w >> MOTION_DEPTH_BITS).astype(np.int32)


RENDER_EXPORTS = ["rodent_hip_scene_create_deforming", "rodent_hip_scene_set_motion_keys", "rodent_hip_scene_motion_keys_status",
                  "rodent_hip_scene_motion_bvh", "rodent_hip_scene_motion_keys",
                  "rodent_hip_scene_create_motion", "rodent_hip_scene_set_motion_transforms", "rodent_hip_scene_motion_instances",
                  "rodent_hip_render_shutter", "rodent_hip_render_shutter_in_effect", "rodent_hip_render_max_path_len_in_effect",
                  "rodent_hip_scene_create_instanced", "rodent_hip_scene_create_flags", "rodent_hip_scene_set_transforms",
                  "rodent_hip_scene_transforms_status", "rodent_hip_scene_instances", "rodent_hip_render_sort_in_effect",
                  "rodent_hip_render_trace_persistent_in_effect",
                  "rodent_hip_scene_deform_prepare", "rodent_hip_scene_deform_device", "rodent_hip_scene_deform_status",
                  "rodent_hip_scene_create","rodent_hip_scene_create_device_bvh", "rodent_hip_scene_create_device_bvh_opt",
                  "rodent_hip_scene_create_device_bvh_split", "rodent_hip_scene_create_device_bvh_ploc",
    "rodent_hip_scene_bvh", "rodent_hip_scene_refit", "rodent_hip_scene_destroy",
    "rodent_hip_scene_refit_prepare", "rodent_hip_scene_refit_device", "rodent_hip_scene_refit_status", "rodent_hip_scene_tables",
    "rodent_hip_render_config", "rodent_hip_render_mapping",
    "rodent_hip_render_capacity", "rodent_hip_render_sort", "rodent_hip_render_hit_records", "rodent_hip_render_overlap",
    "rodent_hip_render_fused_sort", "rodent_hip_render_fused_compact", "rodent_hip_render_mapping_in_effect", "rodent_hip_render_defaults",
    "rodent_hip_render_lds_image", "rodent_hip_render_mega_joint", "rodent_hip_render_trace_persistent", "rodent_hip_render_trace_refill",
    "rodent_hip_render_trace_refill_in_effect", "rodent_hip_render_persist_min_rays", "rodent_hip_render_persist_min_rays_in_effect",
    "rodent_hip_render_trace_kernel_name", "hip_traverse_streams", "get_spp", "render",
                  "setup_interface", "get_pixels", "clear_pixels", "cleanup_interface", "rodent_get_film_data",
                  "rodent_gpu_get_first_primary_stream", "rodent_gpu_get_second_primary_stream", "rodent_gpu_get_secondary_stream",
                  "rodent_gpu_get_tmp_buffer", "rodent_present", "rodent_hip_set_device", "rodent_hip_render_rows",
                      "rodent_hip_render_tiles",
                  "rodent_hip_render_counters", "hip_generate_rays", "hip_traverse_primary", "hip_sort_primary", "hip_shade",
                  "hip_shade_compact", "hip_traverse_secondary", "hip_compact_primary", "hip_bin_primary",
                  "rodent_load_buffer", "rodent_load_bvh2_tri1", "rodent_load_bvh4_tri4", "rodent_load_bvh8_tri4", "rodent_load_png",
                      "rodent_load_jpg",
                  "rodent_cpu_get_primary_stream", "rodent_cpu_get_secondary_stream", "clock_us", "rodent_hip_buffer_size",
                      "rodent_hip_bvh_counts"]

_ready = False


def lib():
    global _ready
    l = abi.lib()
    if not _ready:
        l.rodent_hip_scene_create.argtypes = [i32, C.POINTER(SceneDesc)]; l.rodent_hip_scene_create.restype = None
        l.rodent_hip_scene_destroy.argtypes = [i32]; l.rodent_hip_scene_destroy.restype = None
        l.rodent_hip_scene_create_device_bvh.argtypes = [i32, C.POINTER(SceneDesc), i32]
        l.rodent_hip_scene_create_device_bvh.restype = None
        l.rodent_hip_scene_create_device_bvh_opt.argtypes = [i32, C.POINTER(SceneDesc), C.POINTER(abi.BuildOptions)]
        l.rodent_hip_scene_create_device_bvh_opt.restype = None
        l.rodent_hip_scene_create_device_bvh_split.argtypes = [i32, C.POINTER(SceneDesc), C.POINTER(abi.BuildOptions),
                                                               C.POINTER(abi.SplitOptions)]
        l.rodent_hip_scene_create_device_bvh_split.restype = None
        l.rodent_hip_scene_create_device_bvh_ploc.argtypes = [i32, C.POINTER(SceneDesc), C.POINTER(abi.BuildOptions),
                                                              C.POINTER(abi.SplitOptions), C.POINTER(abi.PlocOptions)]
        l.rodent_hip_scene_create_device_bvh_ploc.restype = None
        l.rodent_hip_scene_bvh.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]
        l.rodent_hip_scene_bvh.restype = None
        l.rodent_hip_scene_refit.argtypes = [i32, vp, vp, vp, vp]; l.rodent_hip_scene_refit.restype = None
        l.rodent_hip_scene_refit_prepare.argtypes = [i32, i32]; l.rodent_hip_scene_refit_prepare.restype = None
        l.rodent_hip_scene_refit_device.argtypes = [i32, vp, vp, vp]; l.rodent_hip_scene_refit_device.restype = None
        l.rodent_hip_scene_refit_status.argtypes = [i32, C.POINTER(i32)]; l.rodent_hip_scene_refit_status.restype = i32
        l.rodent_hip_scene_tables.argtypes = [i32, C.POINTER(SceneTables)]; l.rodent_hip_scene_tables.restype = None
        l.rodent_hip_scene_create_instanced.argtypes = [i32, C.POINTER(SceneDesc), C.POINTER(ObjectRange), i32, vp, i32,
                                                        C.POINTER(abi.BuildOptions)]
        l.rodent_hip_scene_create_instanced.restype = i32
        l.rodent_hip_scene_create_flags.argtypes = [i32]; l.rodent_hip_scene_create_flags.restype = i32
        l.rodent_hip_scene_set_transforms.argtypes = [i32, vp, vp]; l.rodent_hip_scene_set_transforms.restype = None
        l.rodent_hip_scene_transforms_status.argtypes = [i32, C.POINTER(i32)]; l.rodent_hip_scene_transforms_status.restype = i32
        l.rodent_hip_scene_instances.argtypes = [i32, C.POINTER(SceneInstances)]; l.rodent_hip_scene_instances.restype = None
        l.rodent_hip_scene_deform_prepare.argtypes = [i32, C.POINTER(i32), i32, i32]; l.rodent_hip_scene_deform_prepare.restype = i32
        l.rodent_hip_scene_deform_device.argtypes = [i32, vp, vp, vp, vp]; l.rodent_hip_scene_deform_device.restype = None
        l.rodent_hip_scene_deform_status.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
        l.rodent_hip_scene_deform_status.restype = i32
        l.rodent_hip_scene_create_motion.argtypes = [i32, C.POINTER(SceneDesc), C.POINTER(ObjectRange), i32, vp, i32,
                                                     C.POINTER(abi.BuildOptions)]
        l.rodent_hip_scene_create_motion.restype = i32
        l.rodent_hip_scene_set_motion_transforms.argtypes = [i32, vp, vp, vp]; l.rodent_hip_scene_set_motion_transforms.restype = None
        l.rodent_hip_scene_motion_instances.argtypes = [i32, C.POINTER(SceneMotionInstances)]
        l.rodent_hip_scene_motion_instances.restype = None
        l.rodent_hip_scene_create_deforming.argtypes = [i32, C.POINTER(SceneDesc), vp, vp, C.POINTER(abi.BuildOptions)]
        l.rodent_hip_scene_create_deforming.restype = i32
        l.rodent_hip_scene_set_motion_keys.argtypes = [i32, vp, vp, vp, vp, vp]; l.rodent_hip_scene_set_motion_keys.restype = None
        l.rodent_hip_scene_motion_keys_status.argtypes = [i32, C.POINTER(i32)]; l.rodent_hip_scene_motion_keys_status.restype = i32
        l.rodent_hip_scene_motion_bvh.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]
        l.rodent_hip_scene_motion_bvh.restype = None
        l.rodent_hip_scene_motion_keys.argtypes = [i32, C.POINTER(SceneMotionKeys)]; l.rodent_hip_scene_motion_keys.restype = None
        l.rodent_hip_render_shutter.argtypes = [i32, C.c_float, C.c_float]; l.rodent_hip_render_shutter.restype = i32
        l.rodent_hip_render_shutter_in_effect.argtypes = [i32, C.POINTER(C.c_float)]; l.rodent_hip_render_shutter_in_effect.restype = None
        l.rodent_hip_render_max_path_len_in_effect.argtypes = [i32]; l.rodent_hip_render_max_path_len_in_effect.restype = i32
        l.rodent_hip_render_sort_in_effect.argtypes = [i32]; l.rodent_hip_render_sort_in_effect.restype = i32
        l.rodent_hip_render_trace_persistent_in_effect.argtypes = [i32]; l.rodent_hip_render_trace_persistent_in_effect.restype = i32
        l.rodent_hip_render_config.argtypes = [i32, i32, i32]; l.rodent_hip_render_config.restype = None
        l.rodent_hip_render_mapping.argtypes = [i32, i32]; l.rodent_hip_render_mapping.restype = None
        l.rodent_hip_render_capacity.argtypes = [i32, i32]; l.rodent_hip_render_capacity.restype = None
        l.rodent_hip_render_sort.argtypes = [i32, i32]; l.rodent_hip_render_sort.restype = None
        l.rodent_hip_render_overlap.argtypes = [i32, i32]; l.rodent_hip_render_overlap.restype = None
        l.rodent_hip_render_hit_records.argtypes = [i32, i32]; l.rodent_hip_render_hit_records.restype = None
        l.rodent_hip_render_fused_sort.argtypes = [i32, i32]; l.rodent_hip_render_fused_sort.restype = None
        l.rodent_hip_render_lds_image.argtypes = [i32, i32]; l.rodent_hip_render_lds_image.restype = None
        l.rodent_hip_render_fused_compact.argtypes = [i32, i32]; l.rodent_hip_render_fused_compact.restype = None
        l.rodent_hip_render_mapping_in_effect.argtypes = [i32]; l.rodent_hip_render_mapping_in_effect.restype = i32
        l.rodent_hip_render_defaults.argtypes = [i32]; l.rodent_hip_render_defaults.restype = None
        l.rodent_hip_render_trace_persistent.argtypes = [i32, i32]; l.rodent_hip_render_trace_persistent.restype = None
        l.rodent_hip_render_trace_refill.argtypes = [i32, i32, i32]; l.rodent_hip_render_trace_refill.restype = None
        l.rodent_hip_render_trace_refill_in_effect.argtypes = [i32]; l.rodent_hip_render_trace_refill_in_effect.restype = i32
        l.rodent_hip_render_mega_joint.argtypes = [i32, i32]; l.rodent_hip_render_mega_joint.restype = None
        l.rodent_hip_render_persist_min_rays.argtypes = [i32, i32]; l.rodent_hip_render_persist_min_rays.restype = None
        l.rodent_hip_render_persist_min_rays_in_effect.argtypes = [i32]; l.rodent_hip_render_persist_min_rays_in_effect.restype = i32
        l.rodent_hip_render_trace_kernel_name.argtypes = [i32]; l.rodent_hip_render_trace_kernel_name.restype = C.c_char_p
        l.get_spp.argtypes = []; l.get_spp.restype = i32
        l.render.argtypes = [C.POINTER(Settings), i32]; l.render.restype = None
        l.setup_interface.argtypes = [C.c_size_t, C.c_size_t]; l.setup_interface.restype = None
        l.get_pixels.argtypes = []; l.get_pixels.restype = C.POINTER(C.c_float)
        l.clear_pixels.argtypes = []; l.clear_pixels.restype = None
        l.cleanup_interface.argtypes = []; l.cleanup_interface.restype = None
        l.rodent_present.argtypes = [i32]; l.rodent_present.restype = None
        l.rodent_hip_set_device.argtypes = [i32]; l.rodent_hip_set_device.restype = None
        l.rodent_hip_render_rows.argtypes = [i32, C.POINTER(Settings), i32, i32, i32, vp]; l.rodent_hip_render_rows.restype = None
        l.rodent_hip_render_tiles.argtypes = [i32, C.POINTER(Settings), i32, i32, i32, i32, vp]; l.rodent_hip_render_tiles.restype = None
        l.rodent_hip_render_counters.argtypes = [i32, C.POINTER(C.c_uint64)]; l.rodent_hip_render_counters.restype = None
        l.rodent_load_buffer.argtypes = [i32, C.c_char_p]; l.rodent_load_buffer.restype = vp
        for name in ("rodent_load_bvh2_tri1", "rodent_load_bvh4_tri4", "rodent_load_bvh8_tri4"):
            fn = getattr(l, name); fn.argtypes = [i32, C.c_char_p, C.POINTER(vp), C.POINTER(vp)]; fn.restype = None
        for name in ("rodent_load_png", "rodent_load_jpg"):
            fn = getattr(l, name); fn.argtypes = [i32, C.c_char_p, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]; fn.restype = None
        l.rodent_hip_buffer_size.argtypes = [i32, C.c_char_p]; l.rodent_hip_buffer_size.restype = C.c_int64
        l.rodent_hip_bvh_counts.argtypes = [i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32)]; l.rodent_hip_bvh_counts.restype = None
        l.clock_us.argtypes = []; l.clock_us.restype = C.c_int64
        _ready = True
    return l


def scene_desc(scene):
    """(RodentSceneDesc of a scene.Scene-like object, the arrays it points into: keep them alive while the record is used)."""
    keep = [np.ascontiguousarray(getattr(scene, n)) for n in ("vertices", "normals", "face_normals", "indices", "nodes", "tris",
                                                                "materials", "lights", "light_ids", "texcoords", "textures", "texels")]
    desc = SceneDesc(*[a.ctypes.data_as(vp) for a in keep[:9]], len(scene.vertices), scene.num_tris, len(scene.nodes), len(scene.tris),
                     len(scene.materials), len(scene.lights), *[a.ctypes.data_as(vp) for a in keep[9:]], len(scene.textures),
                     len(scene.texels))
    return desc, keep


def create_instanced(dev, scene, ranges, transforms, object_ids, opt=None):
    """rodent_hip_scene_create_instanced as it stands: returns its status (RODENT_SCENE_OK = 0, SCENE_ERR_*) and raises nothing --
    Renderer(instances=...) is the checked way in."""
    from . import formats as F
    desc, keep = scene_desc(scene)
    if not len(scene.nodes):
        desc.nodes = None                                  # (an empty array still has an address)
    if not len(scene.tris):
        desc.tris = None
    ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 4)
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
    descs = np.zeros(len(t), F.INSTANCE_DESC)
    descs["object_to_world"], descs["object"] = t, object_ids
    return lib().rodent_hip_scene_create_instanced(dev, C.byref(desc), ranges.ctypes.data_as(C.POINTER(ObjectRange)), len(ranges),
                                                   descs.ctypes.data_as(vp), len(t), C.byref(opt) if opt is not None else None)


def create_motion(dev, scene, ranges, transforms0, transforms1, object_ids, opt=None):
    """rodent_hip_scene_create_motion as it stands: returns its status and raises nothing -- Renderer(motion=...) is the checked way in."""
    from . import formats as F
    desc, keep = scene_desc(scene)
    if not len(scene.nodes):
        desc.nodes = None
    if not len(scene.tris):
        desc.tris = None
    ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 4)
    t0 = np.ascontiguousarray(transforms0, np.float32).reshape(-1, 12)
    descs = np.zeros(len(t0), F.MOTION_INSTANCE_DESC)
    descs["object_to_world0"], descs["object_to_world1"] = t0, np.ascontiguousarray(transforms1, np.float32).reshape(-1, 12)
    descs["object"] = object_ids
    return lib().rodent_hip_scene_create_motion(dev, C.byref(desc), ranges.ctypes.data_as(C.POINTER(ObjectRange)), len(ranges),
                                                descs.ctypes.data_as(vp), len(t0), C.byref(opt) if opt is not None else None)


def smooth_normals(vertices, indices):
    """(num_vertices, 4) float32 smooth vertex normals by the loader's rule, as rodent_hip_scene_refit_device recomputes them: every
    triangle's face normal c * (1 / |c|), c = (v1 - v0) x (v2 - v0); per vertex those of its corners summed in ascending (triangle,
    corner) order, then normalised where the squared length exceeds FLT_EPSILON, (0, 1, 0) elsewhere.  float32, every operation
    rounded on its own."""
    f32 = np.float32
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 4)
    ix = np.ascontiguousarray(indices, np.int32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        v0, v1, v2 = (v[ix[:, k], :3] for k in range(3))
        a, b = v1 - v0, v2 - v0
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(f32)
        fn = c * (f32(1.0) / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]))[:, None]
        total = np.zeros((len(v), 3), f32)
        np.add.at(total, ix[:, :3].reshape(-1), np.repeat(fn, 3, axis=0))           # unbuffered: one float32 add per corner, in order
        l2 = (total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1]) + total[:, 2] * total[:, 2]
        keep = l2 > np.finfo(f32).eps
        out = np.zeros((len(v), 4), f32)
        out[:, 1] = 1.0
        out[keep, :3] = total[keep] * (f32(1.0) / np.sqrt(l2[keep]))[:, None]
    return out


def create_deforming(dev, scene, vertices1, normals1, opt=None):
    """rodent_hip_scene_create_deforming as it stands: returns its status and raises nothing -- Renderer(deform=...) is the checked way
    in.  vertices1 / normals1: (num_vertices, 4) float32 host tables, or None for a NULL pointer."""
    desc, keep = scene_desc(scene)
    if not len(scene.nodes):
        desc.nodes = None
    if not len(scene.tris):
        desc.tris = None
    tables = [None if t is None else np.ascontiguousarray(t, np.float32) for t in (vertices1, normals1)]
    return lib().rodent_hip_scene_create_deforming(dev, C.byref(desc), *[None if t is None else t.ctypes.data_as(vp) for t in tables],
                                                   C.byref(opt) if opt is not None else None)


def make_settings(cam) -> Settings:
    v = lambda a: Vec3(float(a[0]), float(a[1]), float(a[2]))
    return Settings(v(cam["eye"]), v(cam["dir"]), v(cam["up"]), v(cam["right"]), float(cam["w"]), float(cam["h"]))


class Renderer:
    """One scene on one GPU.  render(cam, iter) accumulates `spp` samples per pixel into the film."""

    MAPPINGS = {"auto": -1, "streaming": 0, "megakernel": 1}       # per scene / mapping_gpu.impala:308-369 / :371-474

    def __init__(self, scene, width, height, spp=4, max_path_len=64, dev=0, mapping="streaming", capacity=0, sort=None, overlap=None,
        fused_sort=None, lds_image=None,
                 trace_persistent=None, fused_compact=None, mega_joint=None, trace_refill=None, hit_records_aos=None, gpu_bvh=None,
                 gpu_bvh_passes=0, gpu_bvh_split=0.0, gpu_bvh_max_pieces=64, gpu_bvh_ploc=0, persist_min_rays=None, instances=None,
                 build=None, motion=None, shutter=(0.0, 1.0), deform=None):
        """Options left at None take the library's default, or what the option's RODENT_HIP_* environment variable says.
        gpu_bvh = max_leaf (1 ... 8): ignore the scene's hierarchy and build one on the device (rodent_hip_scene_create_device_bvh_opt);
        gpu_bvh_passes = 1 ... 3: treelet restructuring passes + SAH leaf collapse on it.
        gpu_bvh_split = (0, 4]: pre-split the triangles into up to that fraction of extra references, at most gpu_bvh_max_pieces per
        triangle (rodent_hip_scene_create_device_bvh_split).
        gpu_bvh_ploc = 1 ... 64: its topology by locally-ordered clustering over that many Morton neighbours to either side
        (rodent_hip_scene_create_device_bvh_ploc); the passes and the split options act on it.
        persist_min_rays: rays from which a traversal launch takes the persistent kernels (rodent_hip_render_persist_min_rays).
        instances = (object_ranges, transforms, object_ids): an INSTANCED scene (rodent_hip_scene_create_instanced) -- `scene` holds the
        concatenated tables of all objects in object space (instances.concat_scenes makes them), object_ranges is (num_objects, 4) int32
        rows first_tri, num_tris, first_light, num_lights, transforms (n, 12) or (n, 3, 4) object_to_world, object_ids n ints; the
        objects' hierarchies are built on the device with build = (max_leaf, treelet_passes) or a gpubuild.options() record (None:
        max_leaf 2, no passes).  A refusal raises gpubuild.BuildError.  Such a scene renders through the streaming loop without the
        sort by material, whatever the options ask for; set_transforms() moves its instances.
        motion = (object_ranges, transforms0, transforms1, object_ids): a MOVING scene (rodent_hip_scene_create_motion) -- an instanced
        scene whose instances carry two placements, at time 0 and at time 1; every path draws a time in `shutter` = (open, close),
        0 <= open <= close <= 1, and sees every instance where that time puts it (entry-wise interpolation of the matrices).  Excludes
        `instances`.  Instances of objects with lights must have equal placements.  Paths are at most 255 vertices long.
        set_motion_transforms() moves both placements, set_shutter() changes the interval.  `shutter` is checked whatever the scene
        (a pair outside 0 <= open <= close <= 1 raises ValueError) but only a moving scene uses it: without `motion` the device keeps
        its default (0, 1).
        deform = (vertices1, normals1): a DEFORMING scene (rodent_hip_scene_create_deforming) -- `scene` is the mesh at time 0 (its
        hierarchy is ignored: the topology is built on the device from key 0 with `build`), vertices1 / normals1 are (num_vertices, 4)
        float32 tables, the mesh at time 1; normals1 = None: smooth normals of key 1 by the loader's rule (smooth_normals), computed
        here on the host.  Every path draws a time in `shutter` and sees every vertex where that time puts it.  Excludes `instances`,
        `motion` and `gpu_bvh`.  The corners of emissive triangles must be equal in both keys.  Paths are at most 255 vertices long.
        set_motion_keys() moves both keys on the device, set_shutter() changes the interval.  A refusal raises gpubuild.BuildError."""
        if deform is not None and instances is not None:
            raise ValueError("deform: a deforming scene is one mesh with two keys (pass `deform` or `instances`, not both)")
        if deform is not None and motion is not None:
            raise ValueError("deform: a deforming scene is one mesh with two keys (pass `deform` or `motion`, not both)")
        if deform is not None and gpu_bvh:
            raise ValueError("deform: the hierarchy is built on the device anyway (pass `build`, not gpu_bvh)")
        if motion is not None and instances is not None:
            raise ValueError("motion: a moving scene carries its own placements (pass `motion` or `instances`, not both)")
        if not 0.0 <= float(shutter[0]) <= float(shutter[1]) <= 1.0:       # (with or without `motion`, before the device is touched)
            raise ValueError(f"shutter: 0 <= open <= close <= 1 is needed, got {tuple(shutter)}")
        if motion is not None and gpu_bvh:
            raise ValueError("motion: the objects' hierarchies are built on the device anyway (pass `build`, not gpu_bvh)")
        if instances is not None and gpu_bvh:
            raise ValueError("instances: the objects' hierarchies are built on the device anyway (pass `build`, not gpu_bvh)")
        if gpu_bvh_passes and not gpu_bvh:
            raise ValueError("gpu_bvh_passes needs gpu_bvh (the treelet passes act on the device-built hierarchy)")
        if gpu_bvh_split and not gpu_bvh:
            raise ValueError("gpu_bvh_split needs gpu_bvh (the split references feed the device-built hierarchy)")
        if gpu_bvh_ploc and not gpu_bvh:
            raise ValueError("gpu_bvh_ploc needs gpu_bvh (the clustering chooses the device-built hierarchy's topology)")
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("rodent_amd: no GPU visible (the renderer has no CPU fallback)")
        self.dev, self.width, self.height, self.spp = dev, width, height, spp
        l = lib()
        keep = [np.ascontiguousarray(getattr(scene, n)) for n in ("vertices", "normals", "face_normals", "indices", "nodes", "tris",
            "materials", "lights", "light_ids")]
        tex = [np.ascontiguousarray(getattr(scene, n)) for n in ("texcoords", "textures", "texels")]
        desc = SceneDesc(*[a.ctypes.data_as(vp) for a in keep], len(scene.vertices), scene.num_tris, len(scene.nodes), len(scene.tris),
                         len(scene.materials), len(scene.lights), *[a.ctypes.data_as(vp) for a in tex], len(scene.textures),
                             len(scene.texels))
        # what update_geometry() compares a moved scene against: the tables a refit leaves alone
        self._fixed = {n: np.array(getattr(scene, n), copy=True) for n in ("indices", "materials", "light_ids", "texcoords", "textures")}
        self._counts = (len(scene.vertices), len(scene.lights), len(scene.texels))
        l.rodent_hip_set_device(dev)
        l.rodent_hip_render_defaults(dev)                    # options of an earlier Renderer in this process do not leak into this one
        self.num_instances = 0
        self.moving = motion is not None
        self.deforming = deform is not None
        if self.deforming:
            self._create_deforming(desc, scene, deform, build)
            self.set_shutter(*shutter)
        elif self.moving:
            ranges, t0, t1, ids = motion
            self._create_instanced(desc, (ranges, t0, ids), build, transforms1=t1)
            self.set_shutter(*shutter)
        elif instances is not None:
            self._create_instanced(desc, instances, build)
        elif gpu_bvh:
            from . import gpubuild
            desc.nodes = desc.tris = None
            desc.num_nodes = desc.num_bvh_tris = 0
            opt = gpubuild.options(int(gpu_bvh), int(gpu_bvh_passes))
            if gpu_bvh_ploc:
                sp = gpubuild.split_options(float(gpu_bvh_split), int(gpu_bvh_max_pieces)) if gpu_bvh_split else None
                pl = gpubuild.ploc_options(int(gpu_bvh_ploc))
                l.rodent_hip_scene_create_device_bvh_ploc(dev, C.byref(desc), C.byref(opt), C.byref(sp) if sp else None, C.byref(pl))
            elif gpu_bvh_split:
                sp = gpubuild.split_options(float(gpu_bvh_split), int(gpu_bvh_max_pieces))
                l.rodent_hip_scene_create_device_bvh_split(dev, C.byref(desc), C.byref(opt), C.byref(sp))
            else:
                l.rodent_hip_scene_create_device_bvh_opt(dev, C.byref(desc), C.byref(opt))
        else:
            l.rodent_hip_scene_create(dev, C.byref(desc))
        l.rodent_hip_render_config(dev, spp, max_path_len)
        l.rodent_hip_render_mapping(dev, self.MAPPINGS[mapping])
        l.rodent_hip_render_capacity(dev, capacity)          # rays per stream, 0 = default (32 Mi)
        # sort hit rays by material before shading (reference behaviour)
        for value, setter in ((sort, l.rodent_hip_render_sort),
                              (overlap, l.rodent_hip_render_overlap),              # shadow rays on a second HIP stream
                              # hit records of the loop's streams as 20-byte records (default) / the ABI's five arrays
                              (hit_records_aos, l.rodent_hip_render_hit_records),
                              # the sort computes a permutation, the shader gathers through it
                              (fused_sort, l.rodent_hip_render_fused_sort),
                              # stream traversal kernels stage the top of the BVH in LDS
                              (lds_image, l.rodent_hip_render_lds_image),
                              # 0 / 1 / 2: 2-wave kernels + second stream / persistent / joint persistent launch (default: per scene)
                              (trace_persistent, l.rodent_hip_render_trace_persistent),
                              # megakernel: shadow ray + next path ray of a lane in one loop (measured slower) / the reference's sequence of
                              # loops (default)
                              (mega_joint, l.rodent_hip_render_mega_joint),
                              # the shader writes continuing rays to their compacted slots
                              (fused_compact, l.rodent_hip_render_fused_compact),
                              # rays from which a lone traversal pass takes the persistent kernels (default 524 288)
                              (persist_min_rays, l.rodent_hip_render_persist_min_rays)):
            if value is not None:
                setter(dev, int(value))
        # persistent traversal launches: lane refill once that many lanes of a wave are idle: n or (bounce rays, shadow rays); 0 = whole
        # chunks
        if trace_refill is not None:
            bounce, shadow = trace_refill if isinstance(trace_refill, (tuple, list)) else (trace_refill, trace_refill)
            l.rodent_hip_render_trace_refill(dev, int(bounce), int(shadow))
        l.setup_interface(width, height)
        l.clear_pixels()

    def _create_instanced(self, desc, instances, build, transforms1=None):
        """transforms1 given: a moving scene (rodent_hip_scene_create_motion), `instances` holding the placements at time 0."""
        from . import formats as F, gpubuild
        ranges, transforms, object_ids = instances
        ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 4)
        t = np.ascontiguousarray(transforms, np.float32)
        n = len(t)
        if t.size != 12 * n:
            raise ValueError(f"instances: expected (n, 12) or (n, 3, 4) transforms, got shape {t.shape}")
        ids = np.ascontiguousarray(object_ids).astype(np.int64).reshape(-1)
        if len(ids) != n:
            raise ValueError(f"instances: {n} transforms but {len(ids)} object ids")
        if transforms1 is None:
            entry = "rodent_hip_scene_create_instanced"
            descs = np.zeros(n, F.INSTANCE_DESC)
            descs["object_to_world"] = t.reshape(n, 12)
        else:
            entry = "rodent_hip_scene_create_motion"
            t1 = np.ascontiguousarray(transforms1, np.float32)
            if t1.size != 12 * n:
                raise ValueError(f"motion: {n} placements at time 0, but transforms1 has shape {t1.shape}")
            descs = np.zeros(n, F.MOTION_INSTANCE_DESC)
            descs["object_to_world0"], descs["object_to_world1"] = t.reshape(n, 12), t1.reshape(n, 12)
        descs["object"] = np.clip(ids, -1, (1 << 31) - 1)                 # (an id past int32 is outside every table too)
        opt = self._build_options(build)
        desc.nodes = desc.tris = None
        desc.num_nodes = desc.num_bvh_tris = 0
        rc = getattr(lib(), entry)(self.dev, C.byref(desc), ranges.ctypes.data_as(C.POINTER(ObjectRange)), len(ranges),
                                   descs.ctypes.data_as(vp), n, C.byref(opt) if opt is not None else None)
        if rc:
            what = SCENE_ERRORS.get(rc, f"status {rc}")
            if rc == SCENE_ERR_DEVICE:
                from .instances import _TLAS_FLAGS
                flags = lib().rodent_hip_scene_create_flags(self.dev)
                what += ": " + (", ".join(s for bit, s in _TLAS_FLAGS if flags > 0 and flags & bit) or f"flags {flags}")
            raise gpubuild.BuildError(f"{entry}: {what}")
        self.num_instances = n

    @staticmethod
    def _build_options(build):
        from . import gpubuild
        if build is None or isinstance(build, abi.BuildOptions):
            return build
        return gpubuild.options(*build) if isinstance(build, (tuple, list)) else gpubuild.options(int(build))

    def _create_deforming(self, desc, scene, deform, build):
        from . import gpubuild
        vertices1, normals1 = deform
        nv = len(scene.vertices)
        v1 = np.ascontiguousarray(vertices1, np.float32)
        if v1.shape != (nv, 4):
            raise ValueError(f"deform: vertices1 must have shape ({nv}, 4), got {v1.shape}")
        n1 = smooth_normals(v1, scene.indices) if normals1 is None else np.ascontiguousarray(normals1, np.float32)
        if n1.shape != (nv, 4):
            raise ValueError(f"deform: normals1 must have shape ({nv}, 4), got {n1.shape}")
        opt = self._build_options(build)
        desc.nodes = desc.tris = None
        desc.num_nodes = desc.num_bvh_tris = 0
        rc = lib().rodent_hip_scene_create_deforming(self.dev, C.byref(desc), v1.ctypes.data_as(vp), n1.ctypes.data_as(vp),
                                                     C.byref(opt) if opt is not None else None)
        if rc:
            what = DEFORMING_ERRORS.get(rc) or SCENE_ERRORS.get(rc, f"status {rc}")
            if rc == SCENE_ERR_DEVICE:
                flags = lib().rodent_hip_scene_create_flags(self.dev)
                what += ": " + self._build_flag_names(flags)
            raise gpubuild.BuildError(f"rodent_hip_scene_create_deforming: {what}")

    @staticmethod
    def _build_flag_names(flags):
        from . import gpubuild
        names = [(gpubuild.NON_FINITE, "non-finite coordinate"), (gpubuild.BAD_INDEX, "vertex index out of range")]
        return ", ".join(s for bit, s in names if flags > 0 and flags & bit) or f"flags {flags}"

    def _no_deforming(self, entry):
        """The entries that work on a flat or an instanced scene refuse a deforming one here: the library aborts on it."""
        if self.deforming:
            from . import gpubuild
            raise gpubuild.BuildError(f"{entry}: the scene is a deforming one (move its keys with set_motion_keys)")

    def set_motion_keys(self, vertices0, vertices1, normals0=None, normals1=None, stream=None, check=True):
        """Both keys of a deforming scene moved (rodent_hip_scene_set_motion_keys): (num_vertices, 4) float32 tensors on the renderer's
        device or integer device pointers; a key may be the scene's own table (motion_key_pointers()), written in place -- then nothing
        is copied -- and the two keys may be one tensor.  normals0 / normals1: both given, or both None: smooth normals recomputed per
        key on the device.  The copies, the normals and the rebuild of the motion records follow on `stream` (a torch stream; None: the
        current one) with no host copy and no wait; the next frame, on any stream, sees the moved keys.  The caller keeps the corners
        of emissive triangles as they were at creation: this call cannot check it.  check=True waits (motion_keys_status) and raises
        gpubuild.BuildError on a flag.  The film is not cleared."""
        import torch
        if not self.deforming:
            raise ValueError("set_motion_keys: the renderer was not made with `deform`")
        if vertices0 is None or vertices1 is None or (normals0 is None) != (normals1 is None):
            raise ValueError("set_motion_keys: both vertex tables are needed, and both tables of normals or neither")
        stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        own = self.motion_key_pointers()
        nv = own["num_vertices"]
        given = (("vertices0", vertices0), ("vertices1", vertices1), ("normals0", normals0), ("normals1", normals1))
        pointers = []
        for name, t in given:
            if t is None or isinstance(t, int):
                pointers.append(t)
                continue
            if not (t.is_cuda and t.data_ptr() == own[name]) and (
                    not t.is_cuda or t.device.index != self.dev or t.dtype != torch.float32 or tuple(t.shape) != (nv, 4)
                    or not t.is_contiguous()):
                raise ValueError(f"set_motion_keys: `{name}` must be a contiguous float32 tensor of shape ({nv}, 4) on cuda:{self.dev} "
                                 "(or an integer device pointer)")
            pointers.append(t.data_ptr())
        tensors = [t for _, t in given if isinstance(t, torch.Tensor)]
        if tensors:
            stream.wait_stream(torch.cuda.current_stream(self.dev))          # the tensors may come from there
        lib().rodent_hip_scene_set_motion_keys(self.dev, *pointers, C.c_void_p(stream.cuda_stream))
        for t in tensors:
            t.record_stream(stream)
        if check:
            self.motion_keys_status(raise_on_flag=True)

    def motion_keys_status(self, raise_on_flag=False):
        """(flags, info words) of the last set_motion_keys, once it has finished (before the first: the creation's); flags 0 = sound
        (gpubuild.NON_FINITE, ...; bit 31: a key's refit completed another node count than the topology's)."""
        words = (i32 * 4)()
        flags = lib().rodent_hip_scene_motion_keys_status(self.dev, words)
        if flags and raise_on_flag:
            from . import gpubuild
            raise gpubuild.BuildError("rodent_hip_scene_set_motion_keys: " + (self._build_flag_names(flags & 0x7FFFFFFF)
                                      if flags & 0x7FFFFFFF else f"malformed hierarchy ({words[0]}, {words[3]} nodes completed)"))
        return flags, list(words)

    def motion_key_pointers(self):
        """Device pointers (integers) of a deforming scene's key tables (rodent_hip_scene_motion_keys) and num_vertices."""
        t = SceneMotionKeys()
        lib().rodent_hip_scene_motion_keys(self.dev, C.byref(t))
        return {n: (getattr(t, n) or 0) for n, _ in SceneMotionKeys._fields_}

    def motion_key_tensor(self, name):
        """One of the scene's own key tables ("vertices0", "vertices1", "normals0", "normals1") as a (num_vertices, 4) float32 torch
        tensor that shares its memory: write it in place, then pass it to set_motion_keys (nothing is copied)."""
        import torch
        p = self.motion_key_pointers()

        class Table:
            __cuda_array_interface__ = {"shape": (p["num_vertices"], 4), "typestr": "<f4", "data": (p[name], False), "version": 2,
                                        "strides": None}
        return torch.as_tensor(Table(), device=f"cuda:{self.dev}")

    def deforming_tables(self):
        """Host copies (numpy) of what a deforming scene holds: vertices0, vertices1, normals0, normals1 ((num_vertices, 4) float32),
        motion_nodes (MOTION_NODE2), motion_tris (MOTION_TRI1), lights (scene.LIGHT) and info (the last motion build's info words).
        Waits for the device."""
        import torch
        from . import formats as F
        from .scene import LIGHT
        p = self.motion_key_pointers()
        nodes, tris, nn, nt = vp(), vp(), i32(), i32()
        lib().rodent_hip_scene_motion_bvh(self.dev, C.byref(nodes), C.byref(tris), C.byref(nn), C.byref(nt))
        scene = self.scene_table_pointers()
        torch.cuda.synchronize(self.dev)
        hip = C.cdll.LoadLibrary("libamdhip64.so")

        def fetch(ptr, dtype, count, shape=None):
            nbytes = count * np.dtype(dtype).itemsize
            t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=f"cuda:{self.dev}")
            hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3)
            a = t.cpu().numpy()[:nbytes].view(dtype).copy()
            return a.reshape(shape) if shape else a
        nv = p["num_vertices"]
        out = {n: fetch(p[n], "<f4", 4 * nv, (nv, 4)) for n in ("vertices0", "vertices1", "normals0", "normals1")}
        out.update(motion_nodes=fetch(nodes.value, F.MOTION_NODE2, nn.value), motion_tris=fetch(tris.value, F.MOTION_TRI1, nt.value),
                   lights=fetch(scene["lights"], LIGHT, scene["num_lights"]), info=fetch(p["info"], "<i4", 4))
        return out

    def _matrices_pointer(self, t, what):
        """Device pointer of num_instances x 12 float32 entries given as a tensor on the renderer's device, or as an integer pointer."""
        import torch
        if isinstance(t, int):
            return t
        if (not t.is_cuda or t.device.index != self.dev or t.dtype != torch.float32 or t.numel() != 12 * self.num_instances
                or not t.is_contiguous()):
            raise ValueError(f"{what}: a contiguous float32 tensor of {self.num_instances} x 12 entries on cuda:{self.dev} is needed (or "
                             "an integer device pointer)")
        return t.data_ptr()

    def set_motion_transforms(self, transforms0, transforms1, stream=None, check=True):
        """Both placements of a moving scene's instances moved (rodent_hip_scene_set_motion_transforms): two tensors as for
        set_transforms (they may be the same one), the placements at time 0 and at time 1.  The motion TLAS, the instance array, slot_of
        and the world lights (from the placements at time 0) follow on `stream` with no host copy and no wait.  The caller keeps the two
        placements of every instance of an object with lights equal: this call cannot check it.  check=True waits
        (transforms_status) and raises gpubuild.BuildError on a flag (a singular or non-finite endpoint).  The film is not cleared."""
        import torch
        self._no_deforming("set_motion_transforms")
        stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        pointers = [self._matrices_pointer(t, "set_motion_transforms") for t in (transforms0, transforms1)]
        tensors = [t for t in (transforms0, transforms1) if not isinstance(t, int)]
        if tensors:
            stream.wait_stream(torch.cuda.current_stream(self.dev))          # the tensors may come from there
        lib().rodent_hip_scene_set_motion_transforms(self.dev, *pointers, C.c_void_p(stream.cuda_stream))
        for t in tensors:
            t.record_stream(stream)
        if check:
            self.transforms_status(raise_on_flag=True)

    def set_shutter(self, open_, close):
        """The interval a moving scene's paths draw their times in (rodent_hip_render_shutter): 0 <= open <= close <= 1, else ValueError
        and nothing changes.  A path's time is min(close, open + (close - open) * u) in float32, u its shutter sample."""
        if lib().rodent_hip_render_shutter(self.dev, float(open_), float(close)) != 0:
            raise ValueError(f"shutter: 0 <= open <= close <= 1 is needed, got ({open_}, {close})")

    def shutter(self):
        out = (C.c_float * 2)()
        lib().rodent_hip_render_shutter_in_effect(self.dev, out)
        return float(out[0]), float(out[1])

    def max_path_len(self):
        """The path length the next frame uses (rodent_hip_render_max_path_len_in_effect): at most 255 with a moving scene loaded."""
        return lib().rodent_hip_render_max_path_len_in_effect(self.dev)

    def motion_pointers(self):
        """Device pointers (integers) and counts of a moving scene's tables (rodent_hip_scene_motion_instances)."""
        t = SceneMotionInstances()
        lib().rodent_hip_scene_motion_instances(self.dev, C.byref(t))
        return {n: (getattr(t, n) or 0) for n, _ in SceneMotionInstances._fields_}

    def motion_tables(self):
        """instance_tables() of a moving scene: `instances` are MOTION_INSTANCE records, `descs` MOTION_INSTANCE_DESC records."""
        from . import formats as F
        return self._derived_tables(self.motion_pointers(), F.MOTION_INSTANCE, F.MOTION_INSTANCE_DESC)

    def set_transforms(self, transforms, stream=None, check=True):
        """The instances moved (rodent_hip_scene_set_transforms): `transforms` is a contiguous float32 tensor of num_instances x 12
        object_to_world entries ((n, 12) or (n, 3, 4)) on the renderer's device, or an integer device pointer.  The top-level hierarchy,
        the instance array, slot_of and the world lights follow on `stream` (a torch stream; None: the current one) with no host copy
        and no wait; the next frame, on any stream, sees the moved instances.  check=True waits for the rebuild
        (rodent_hip_scene_transforms_status) and raises gpubuild.BuildError on a flag (a singular or non-finite matrix): the scene must
        not be rendered before a sound rebuild.  The film is not cleared."""
        import torch
        self._no_deforming("set_transforms")
        stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        if isinstance(transforms, int):
            pointer = transforms
        else:
            t = transforms
            if (not t.is_cuda or t.device.index != self.dev or t.dtype != torch.float32 or t.numel() != 12 * self.num_instances
                    or not t.is_contiguous()):
                raise ValueError(f"set_transforms: a contiguous float32 tensor of {self.num_instances} x 12 entries on cuda:{self.dev} is "
                                 "needed (or an integer device pointer)")
            stream.wait_stream(torch.cuda.current_stream(self.dev))          # the tensor may come from there
            pointer = t.data_ptr()
        lib().rodent_hip_scene_set_transforms(self.dev, pointer, C.c_void_p(stream.cuda_stream))
        if not isinstance(transforms, int):
            transforms.record_stream(stream)
        if check:
            self.transforms_status(raise_on_flag=True)

    def transforms_status(self, raise_on_flag=False):
        """(flags, info words) of the last set_transforms, once it has finished (before the first: the creation's); flags 0 = sound."""
        words = (i32 * 4)()
        flags = lib().rodent_hip_scene_transforms_status(self.dev, words)
        if flags and raise_on_flag:
            from . import gpubuild
            from .instances import _TLAS_FLAGS
            raise gpubuild.BuildError("rodent_hip_scene_set_transforms: " + ", ".join(s for bit, s in _TLAS_FLAGS if flags & bit))
        return flags, list(words)

    def prepare_deform(self, objects, smooth_normals=True):
        """Declares the deforming set of an instanced scene (rodent_hip_scene_deform_prepare): `objects` are object ids, any order,
        none twice.  One-time and synchronous: allocates what deform_objects needs (smooth_normals: also what a call without `normals`
        needs); calling it again replaces the set.  A refusal raises gpubuild.BuildError and leaves the scene as it is."""
        ids = np.ascontiguousarray(np.clip(np.asarray(objects, np.int64).reshape(-1), -1, (1 << 31) - 1).astype(np.int32))
        rc = lib().rodent_hip_scene_deform_prepare(self.dev, ids.ctypes.data_as(C.POINTER(i32)), len(ids), int(bool(smooth_normals)))
        if rc:
            from . import gpubuild
            what = {SCENE_ERR_NOT_INSTANCED: "no instanced scene is loaded", SCENE_ERR_COUNTS: "no objects listed",
                    SCENE_ERR_OBJECT: "an object id outside the table, or one listed twice"}.get(rc, f"status {rc}")
            raise gpubuild.BuildError(f"rodent_hip_scene_deform_prepare: {what}")

    def deform_objects(self, vertices, normals=None, transforms=None, stream=None, check=True):
        """The vertices of the deforming objects moved (rodent_hip_scene_deform_device): `vertices` -- and `normals`, or None for smooth
        normals recomputed for the set's vertices -- are the whole concatenated (num_vertices, 4) float32 tables as tensors on the
        renderer's device or integer device pointers (the scene's own vertex table, scene_vertices_tensor(), written in place, is
        copied nowhere); rows no listed object names must equal the scene's.  transforms: None, or the instances' new matrices as for
        set_transforms -- they move in the same call, with one rebuild of the top-level hierarchy.  The listed objects' face normals,
        light records, vertex normals, hierarchies and shading records, then the top-level hierarchy, slot_of and the world lights
        follow on `stream` (a torch stream; None: the current one) with no host copy and no wait; the next frame, on any stream, sees
        the deformed scene.  check=True waits (deform_status) and raises gpubuild.BuildError on a flag.  The film is not cleared."""
        import torch
        self._no_deforming("deform_objects")
        stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        tensors = [t for t in (vertices, normals, transforms) if isinstance(t, torch.Tensor)]
        pointers = [self._table_pointer(vertices, "vertices"), self._table_pointer(normals, "normals")]
        if pointers[0] is None:
            raise ValueError("deform_objects: `vertices` is None")
        if isinstance(transforms, torch.Tensor):
            t = transforms
            if (not t.is_cuda or t.device.index != self.dev or t.dtype != torch.float32 or t.numel() != 12 * self.num_instances
                    or not t.is_contiguous()):
                raise ValueError(f"deform_objects: `transforms` must be a contiguous float32 tensor of {self.num_instances} x 12 entries "
                                 f"on cuda:{self.dev} (or an integer device pointer)")
            pointers.append(t.data_ptr())
        else:
            pointers.append(transforms)
        if tensors:
            stream.wait_stream(torch.cuda.current_stream(self.dev))          # the tensors may come from there
        lib().rodent_hip_scene_deform_device(self.dev, *pointers, C.c_void_p(stream.cuda_stream))
        for t in tensors:
            t.record_stream(stream)
        if check:
            self.deform_status(raise_on_flag=True)

    def deform_status(self, raise_on_flag=False):
        """(flags, refit info words, TLAS info words) of the last deform_objects, once it has finished: flags 0 = sound (the refit's
        flags | the top-level build's; bit 31: nodes the refit could not complete)."""
        refit, tlas = (i32 * 4)(), (i32 * 4)()
        flags = lib().rodent_hip_scene_deform_status(self.dev, refit, tlas)
        if flags and raise_on_flag:
            from . import gpubuild
            from .instances import _TLAS_FLAGS
            raise gpubuild.BuildError("rodent_hip_scene_deform_device: " + (", ".join(s for bit, s in _TLAS_FLAGS if flags & bit)
                                      or f"malformed hierarchy ({refit[0]} nodes completed)"))
        return flags, list(refit), list(tlas)

    def instance_pointers(self):
        """Device pointers (integers) and counts of an instanced scene's tables (rodent_hip_scene_instances)."""
        t = SceneInstances()
        lib().rodent_hip_scene_instances(self.dev, C.byref(t))
        return {n: (getattr(t, n) or 0) for n, _ in SceneInstances._fields_}

    def instance_tables(self):
        """Host copies (numpy) of what an instanced scene derives: tlas_nodes (NODE2), instances (INSTANCE, leaf order), descs
        (INSTANCE_DESC), objects (OBJECT), slot_of, bases ((n, 2) int32), light_owner, lights (the world lights, scene.LIGHT),
        object_lights and tlas_info (the last rebuild's info words).  Waits for the device."""
        from . import formats as F
        return self._derived_tables(self.instance_pointers(), F.INSTANCE, F.INSTANCE_DESC)

    def _derived_tables(self, p, instance_dtype, desc_dtype):
        import torch
        from . import formats as F
        from .scene import LIGHT
        torch.cuda.synchronize(self.dev)
        hip = C.cdll.LoadLibrary("libamdhip64.so")

        def fetch(name, dtype, count, shape=None):
            nbytes = count * np.dtype(dtype).itemsize
            t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=f"cuda:{self.dev}")
            hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(p[name]), C.c_size_t(nbytes), 3)
            a = t.cpu().numpy()[:nbytes].view(dtype).copy()
            return a.reshape(shape) if shape else a
        n = p["num_instances"]
        info = fetch("tlas_info", "<i4", 4)
        return {"tlas_nodes": fetch("tlas_nodes", F.NODE2, int(info[0])), "instances": fetch("instances", instance_dtype, n),
                "descs": fetch("descs", desc_dtype, n), "objects": fetch("objects", F.OBJECT, p["num_objects"]),
                "slot_of": fetch("slot_of", "<i4", n), "bases": fetch("bases", "<i4", 2 * n, (n, 2)),
                "light_owner": fetch("light_owner", "<i4", p["num_lights"]), "lights": fetch("lights", LIGHT, p["num_lights"]),
                "object_lights": fetch("object_lights", LIGHT, p["num_object_lights"]), "tlas_info": info}

    def options_in_effect(self):
        """What the next frame uses for the scene that is loaded: mapping name, trace_persistent, (refill thresholds), sort.
        The keys depend on how the renderer was made: one made with `motion=` or `deform=` ALSO returns max_path_len and shutter; every other
        renderer returns exactly the four keys above (callers compare that dictionary for equality), and max_path_len() and
        shutter() read the two values for any renderer."""
        l = lib()
        out = {"mapping": self.mapping_name(), "trace_persistent": l.rodent_hip_render_trace_persistent_in_effect(self.dev),
               "trace_refill": self.trace_refill(), "sort": l.rodent_hip_render_sort_in_effect(self.dev)}
        if self.moving or self.deforming:
            out.update(max_path_len=self.max_path_len(), shutter=self.shutter())
        return out

    def configure(self, spp, max_path_len):
        self.spp = spp
        lib().rodent_hip_render_config(self.dev, spp, max_path_len)

    def mapping_name(self):
        """The mapping the next frame uses ("streaming" / "megakernel"): the caller's choice, or the library's for this scene."""
        return {0: "streaming", 1: "megakernel"}[lib().rodent_hip_render_mapping_in_effect(self.dev)]

    def trace_refill(self):
        """(idle lanes that trigger a refill while a wave draws bounce rays, ... shadow rays) of the persistent traversal launches; (0, 0) =
        whole chunks."""
        v = lib().rodent_hip_render_trace_refill_in_effect(self.dev)
        return v & 255, v >> 8

    def persist_min_rays(self, rays=None):
        """Sets (rays given; < 0 = the default, 524 288) and returns the ray count from which a traversal launch takes the persistent
        kernels (rodent_hip_render_persist_min_rays)."""
        if rays is not None:
            lib().rodent_hip_render_persist_min_rays(self.dev, int(rays))
        return lib().rodent_hip_render_persist_min_rays_in_effect(self.dev)

    def trace_kernel_name(self):
        """The main kernel of the newest stream traversal launch on this device, e.g. "k_trace_refill<1,true>"."""
        return lib().rodent_hip_render_trace_kernel_name(self.dev).decode()

    def clear(self):
        lib().clear_pixels()

    def render(self, cam, iter_):
        st = make_settings(cam)
        lib().render(C.byref(st), iter_)

    def render_rows(self, cam, iter_, y0, y1):
        st = make_settings(cam)
        lib().rodent_hip_render_rows(self.dev, C.byref(st), iter_, y0, y1, None)

    def render_tiles(self, cam, iter_, tile_rows, first_tile, tile_stride):
        """The interleaved row tiles first_tile, first_tile + tile_stride, ... of tile_rows rows each (GPU k of K: first_tile = k,
        tile_stride = K)."""
        st = make_settings(cam)
        lib().rodent_hip_render_tiles(self.dev, C.byref(st), iter_, tile_rows, first_tile, tile_stride, None)

    def film(self):
        lib().rodent_present(self.dev)
        p = lib().get_pixels()
        return np.ctypeslib.as_array(p, shape=(self.height, self.width, 3)).copy()

    def counters(self):
        buf = (C.c_uint64 * 4)()
        lib().rodent_hip_render_counters(self.dev, buf)
        return {"primary_rays": buf[0], "shadow_rays": buf[1], "iterations": buf[2], "generated": buf[3]}

    def scene_bvh(self):
        """Host copies (nodes NODE2, tris TRI1) of the hierarchy the scene traces (rodent_hip_scene_bvh)."""
        import torch
        nodes, tris, nn, nt = vp(), vp(), i32(), i32()
        lib().rodent_hip_scene_bvh(self.dev, C.byref(nodes), C.byref(tris), C.byref(nn), C.byref(nt))
        out = []
        for ptr, count, dt in ((nodes, nn.value, abi.F.NODE2), (tris, nt.value, abi.F.TRI1)):
            t = torch.empty(max(count, 1) * dt.itemsize, dtype=torch.uint8, device=f"cuda:{self.dev}")
            torch.cuda.synchronize(self.dev)
            C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(t.data_ptr()), ptr, C.c_size_t(count * dt.itemsize), 3)
            out.append(t.cpu().numpy()[: count * dt.itemsize].view(dt).copy())
        return tuple(out)

    def update_geometry(self, scene):
        """The scene's vertices moved: `scene` is a Scene with the same index table (and the same materials, light ids and textures)
        and new vertices, normals, face normals and lights.  Overwrites the device tables, refits the hierarchy in place and rebuilds
        what depends on positions (rodent_hip_scene_refit); synchronous.  The film is not cleared."""
        self._no_deforming("update_geometry")
        if (len(scene.vertices), len(scene.lights), len(scene.texels)) != self._counts:
            raise ValueError("update_geometry: the scene's vertex, light or texel count differs from the one the renderer was created with")
        for n, mine in self._fixed.items():
            theirs = np.asarray(getattr(scene, n))
            if theirs.shape != mine.shape or theirs.tobytes() != mine.tobytes():
                raise ValueError(f"update_geometry: the scene's `{n}` table differs from the one the renderer was created with")
        tables = [np.ascontiguousarray(getattr(scene, n)) for n in ("vertices", "normals", "face_normals", "lights")]
        lib().rodent_hip_scene_refit(self.dev, *[a.ctypes.data_as(vp) for a in tables])

    def prepare_update(self, smooth_normals=True):
        """One-time allocations of update_geometry_device (rodent_hip_scene_refit_prepare), so that its first call allocates nothing
        either; smooth_normals: also the incidence lists a call without `normals` needs."""
        self._no_deforming("prepare_update")
        lib().rodent_hip_scene_refit_prepare(self.dev, int(bool(smooth_normals)))

    def _table_pointer(self, t, what):
        """Device pointer of a (num_vertices, 4) float32 table given as a tensor on the renderer's device, or as an integer pointer."""
        if t is None or isinstance(t, int):
            return t
        if t.is_cuda and t.data_ptr() == self.scene_table_pointers()[what]:
            return t.data_ptr()                              # the scene's own table (scene_vertices_tensor)
        nv = self._counts[0]
        if (not t.is_cuda or t.device.index != self.dev or str(t.dtype) != "torch.float32" or tuple(t.shape) != (nv, 4)
                or not t.is_contiguous()):
            raise ValueError(f"update_geometry_device: `{what}` must be a contiguous float32 tensor of shape ({nv}, 4) on cuda:{self.dev} "
                             "(or an integer device pointer)")
        return t.data_ptr()

    def update_geometry_device(self, vertices, normals=None, stream=None, check=True):
        """The scene's vertices moved and already live on the device (rodent_hip_scene_refit_device): `vertices` -- and `normals`, or
        None for smooth normals recomputed from the faces -- are (num_vertices, 4) float32 tensors on the renderer's device, or integer
        device pointers (the scene's own vertex table, scene_table_pointers()["vertices"], written in place, is copied nowhere).  Face
        normals, light records, the hierarchy's boxes and Tri1 records, both LDS top images and the shading records follow on `stream`
        (a torch stream; None: the current one), with no host copy and no wait; the next frame, on any stream, sees the moved scene.
        check=True waits for the refit (rodent_hip_scene_refit_status) and raises gpubuild.BuildError on a flag: a non-finite
        coordinate, a malformed hierarchy.  The film is not cleared."""
        import torch
        self._no_deforming("update_geometry_device")
        stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        tensors = [t for t in (vertices, normals) if isinstance(t, torch.Tensor)]
        pointers = (self._table_pointer(vertices, "vertices"), self._table_pointer(normals, "normals"))
        if pointers[0] is None:
            raise ValueError("update_geometry_device: `vertices` is None")
        if tensors:
            stream.wait_stream(torch.cuda.current_stream(self.dev))          # the tensors may come from there
        lib().rodent_hip_scene_refit_device(self.dev, *pointers, C.c_void_p(stream.cuda_stream))
        for t in tensors:
            t.record_stream(stream)
        if check:
            self.update_status(raise_on_flag=True)

    def update_status(self, raise_on_flag=False):
        """(flags, info words) of the last update_geometry_device, once it has finished: flags 0 = sound (gpubuild.NON_FINITE, ...; bit
        31: nodes the refit could not complete)."""
        words = (i32 * 4)()
        flags = lib().rodent_hip_scene_refit_status(self.dev, words)
        if flags and raise_on_flag:
            from . import gpubuild
            gpubuild._raise_flags("rodent_hip_scene_refit_device", words)
            raise gpubuild.BuildError(f"rodent_hip_scene_refit_device: malformed hierarchy ({words[0]} nodes completed)")
        return flags, list(words)

    def scene_table_pointers(self):
        """Device pointers (integers; 0 = the scene has no such table) and counts of the tables the scene owns (rodent_hip_scene_tables)."""
        t = SceneTables()
        lib().rodent_hip_scene_tables(self.dev, C.byref(t))
        return {n: (getattr(t, n) or 0) for n, _ in SceneTables._fields_}

    def scene_vertices_tensor(self):
        """The scene's own vertex table as a (num_vertices, 4) float32 torch tensor that shares its memory: write it in place with torch
        ops, then pass it to update_geometry_device (nothing is copied).  Valid until the scene is destroyed."""
        import torch
        p = self.scene_table_pointers()

        class Table:
            __cuda_array_interface__ = {"shape": (p["num_vertices"], 4), "typestr": "<f4", "data": (p["vertices"], False), "version": 2,
                                        "strides": None}
        return torch.as_tensor(Table(), device=f"cuda:{self.dev}")

    def scene_tables(self):
        """Host copies (numpy) of the tables the scene derives from positions: vertices, normals, face_normals (float32, 4 columns),
        lights (scene.LIGHT), tri_shade ((num_tris, 12) float32, or None) and the two LDS top images ((records, 16) int32)."""
        import torch
        from .scene import LIGHT
        p = self.scene_table_pointers()
        torch.cuda.synchronize(self.dev)
        hip = C.cdll.LoadLibrary("libamdhip64.so")

        def fetch(ptr, dtype, count, shape):
            if not ptr:
                return None
            nbytes = count * np.dtype(dtype).itemsize
            t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=f"cuda:{self.dev}")
            hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3)
            return t.cpu().numpy()[:nbytes].view(dtype).reshape(shape).copy()
        nv, nt = p["num_vertices"], p["num_tris"]
        return {"vertices": fetch(p["vertices"], "<f4", 4 * nv, (nv, 4)), "normals": fetch(p["normals"], "<f4", 4 * nv, (nv, 4)),
                "face_normals": fetch(p["face_normals"], "<f4", 4 * nt, (nt, 4)),
                "lights": fetch(p["lights"], LIGHT, p["num_lights"], (p["num_lights"],)),
                "tri_shade": fetch(p["tri_shade"], "<f4", 12 * nt, (nt, 12)),
                "top_image": fetch(p["top_image"], "<i4", 16 * p["top_nodes"], (p["top_nodes"], 16)),
                "top_image_large": fetch(p["top_image_large"], "<i4", 16 * p["top_nodes_large"], (p["top_nodes_large"], 16))}

    def close(self):
        lib().rodent_hip_scene_destroy(self.dev)
        lib().cleanup_interface()


def tonemap(film, iters):
    """(film / iter)^(1/2.2), clamp, x255 -- src/driver/driver.cpp:144-157."""
    x = np.clip(np.power(np.maximum(film / np.float32(iters), 0), np.float32(1 / 2.2)), 0, 1)
    return (x * 255.0).astype(np.uint8)


# ---- stage-level API (the reference's device kernels as separate entry points) ----------------
class RayStream(C.Structure):
    _fields_ = [(n, vp) for n in ("id", "org_x", "org_y", "org_z", "dir_x", "dir_y", "dir_z", "tmin", "tmax")]


class PrimaryStream(C.Structure):
    _fields_ = [("rays", RayStream)] + [(n, vp) for n in ("geom_id", "prim_id", "t", "u", "v", "rnd", "mis", "contrib_r", "contrib_g",
        "contrib_b", "depth")] + \
               [("size", i32), ("pad", i32)]


class SecondaryStream(C.Structure):
    _fields_ = [("rays", RayStream)] + [(n, vp) for n in ("prim_id", "color_r", "color_g", "color_b")] + [("size", i32), ("pad", i32)]


def stage_lib():
    l = lib()
    l.rodent_gpu_get_first_primary_stream.argtypes = [i32, C.POINTER(PrimaryStream),
        i32]; l.rodent_gpu_get_first_primary_stream.restype = None
    l.rodent_gpu_get_second_primary_stream.argtypes = [i32, C.POINTER(PrimaryStream),
        i32]; l.rodent_gpu_get_second_primary_stream.restype = None
    l.rodent_gpu_get_secondary_stream.argtypes = [i32, C.POINTER(SecondaryStream), i32]; l.rodent_gpu_get_secondary_stream.restype = None
    l.rodent_get_film_data.argtypes = [i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]; l.rodent_get_film_data.restype = None
    l.hip_generate_rays.argtypes = [i32, C.POINTER(PrimaryStream), i32, i32, i32, C.POINTER(Settings), i32, i32, i32, i32, i32,
        vp]; l.hip_generate_rays.restype = None
    l.hip_traverse_primary.argtypes = [i32, C.POINTER(PrimaryStream), vp]; l.hip_traverse_primary.restype = None
    l.hip_sort_primary.argtypes = [i32, C.POINTER(PrimaryStream), C.POINTER(PrimaryStream), C.POINTER(i32),
        vp]; l.hip_sort_primary.restype = None
    l.hip_shade.argtypes = [i32, C.POINTER(PrimaryStream), C.POINTER(SecondaryStream), i32, vp]; l.hip_shade.restype = None
    l.hip_shade_compact.argtypes = [i32, C.POINTER(PrimaryStream), C.POINTER(PrimaryStream), C.POINTER(SecondaryStream), vp, i32, i32, i32,
        vp]; l.hip_shade_compact.restype = i32
    l.hip_traverse_secondary.argtypes = [i32, C.POINTER(SecondaryStream), vp]; l.hip_traverse_secondary.restype = None
    l.hip_traverse_streams.argtypes = [i32, C.POINTER(PrimaryStream), i32, C.POINTER(SecondaryStream), vp, i32, vp]
    l.hip_traverse_streams.restype = i32
    l.hip_compact_primary.argtypes = [i32, C.POINTER(PrimaryStream), C.POINTER(PrimaryStream), vp]; l.hip_compact_primary.restype = i32
    l.hip_bin_primary.argtypes = [i32, C.POINTER(PrimaryStream), C.POINTER(PrimaryStream), i32, i32, i32, i32, i32, vp, vp, i32,
        C.POINTER(i32), vp]; l.hip_bin_primary.restype = i32
    return l


def write_stream_array(ptr, values):
    """Copies a host array of 4-byte words into one stream array (device pointer)."""
    import torch
    a = np.ascontiguousarray(values)
    assert a.dtype.itemsize == 4
    if a.size == 0:
        return
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    abi.lib()
    C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(ptr), C.c_void_p(t.data_ptr()), C.c_size_t(a.nbytes), 3)
    torch.cuda.synchronize()


def read_stream_array(ptr, count, dtype):
    """Copies `count` words of one stream array (device pointer) to the host."""
    import torch
    if count == 0:
        return np.zeros(0, dtype)
    nbytes = count * 4
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    abi.lib()  # same process / same HIP runtime
    C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3)
    return t.cpu().numpy().view(dtype).copy()
