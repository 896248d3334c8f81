"""Instanced scenes: many placed copies of a few objects, traced through a two-level hierarchy built on the GPU (C ABI:
include/rodent_instances.h; kernels: csrc/build_tlas.h, csrc/traversal_instanced.h).

    objects = pack_objects([bvh_a, bvh_b])                    # width-2 DeviceBvhs (any builder) or (nodes, tris) numpy pairs
    tlas = build_tlas(objects, transforms, object_ids)        # transforms: (n, 12) or (n, 3, 4), row-major object_to_world
    hits, ids = trace(objects, tlas, rays)                    # Hit1 records (tri_id: the object's own prim id) + instance ids
    build_tlas(objects, moved_transforms, object_ids, out=tlas)   # the per-frame path: the objects' hierarchies stay as they are
    refit_objects(objects, [2, 0], moved_vertices, indices, rows) # geometry moved inside objects 2 and 0: refitted in one launch list
    objects = build_objects(vertices, indices, rows)              # ALL objects built on the device in one launch list: pack_objects of
                                                                  # per-object gpubuild.build_bvh2, byte for byte
    slotted = build_objects(vertices, indices, rows, slots=True)  # ... each in a node slot of its own, so that
    rebuild_objects(slotted, [2, 0], moved_vertices, indices, rows[[2, 0]])   # rebuilds objects 2 and 0 where they lie (new topologies)
    moving = build_motion_tlas(objects, transforms0, transforms1, object_ids)     # every copy placed at time 0 and at time 1 ...
    hits, ids = trace_motion(objects, moving, rays, times)                        # ... and every ray traced at its own time
    deforming = build_motion_objects(objects, vertices0, vertices1, indices, rows)    # every object at time 0 and at time 1 too:
    moving = build_motion_tlas(deforming, transforms0, transforms1, object_ids)       # a MotionObjectSet goes where an ObjectSet goes,
    hits, ids = trace_motion(deforming, moving, rays, times)                          # one time per ray through both levels

The top-level hierarchy is a pure function of the objects' root boxes, the transforms and max_leaf, byte for byte.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi, formats as F
from .gpubuild import BuildError, INFO_WORDS, MAX_LEAF, _FLAGS, _enqueue

MAX_INSTANCES = 1 << 22
BAD_OBJECT, BAD_TRANSFORM = 8, 16
ERR_NUM_INSTANCES, ERR_NUM_OBJECTS = -14, -15              # RODENT_TLAS_ERR_*
_TLAS_FLAGS = _FLAGS + ((BAD_OBJECT, "object index outside the object table"),
                        (BAD_TRANSFORM, "singular or non-finite transform"))


def _need_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")


class ObjectSet:
    """The packed objects: every object's Node2 records in `nodes`, every object's Tri1 records in `tris` (views of ONE allocation,
    `buffer`, the triangles 256-byte aligned behind the nodes, as in abi.DeviceBvh), and the RodentObject table on the host (`table`,
    formats.OBJECT) and on the device (`table_dev`)."""

    def __init__(self, buffer, nodes, tris, table, table_dev, dev, capacities=None, depths=None):
        self.buffer, self.nodes, self.tris, self.table, self.table_dev, self.dev = buffer, nodes, tris, table, table_dev, dev
        self.num_objects, self.num_nodes, self.num_tris = len(table), int(table["num_nodes"].sum()), int(table["num_tris"].sum())
        # capacities: per object the Node2 records of its slot (build_objects(slots=True): rebuild_objects works in such a set); None
        # for a tight set.  depths: per object its hierarchy's depth, where the builder reported it (build_objects).
        self.capacities, self.depths = capacities, depths

    @property
    def device_bytes(self):
        return self.buffer.numel() + self.table_dev.numel() * self.table_dev.element_size()


def pack_objects(bvhs, dev=0) -> ObjectSet:
    """Packs width-2 abi.DeviceBvh objects or (nodes NODE2, tris TRI1) numpy pairs into one ObjectSet.  Child ids and leaf indices stay
    relative to each object's own first node and triangle: packing is concatenation, no id is rewritten."""
    _need_gpu()
    if not len(bvhs):
        raise ValueError("pack_objects: at least one object is needed")
    cuda = f"cuda:{dev}"
    parts, table = [], np.zeros(len(bvhs), F.OBJECT)
    for k, b in enumerate(bvhs):
        if isinstance(b, abi.DeviceBvh):
            if b.width != 2:
                raise ValueError("pack_objects: BVH2 / Tri1 hierarchies are needed")
            nb = b.nodes.view(torch.uint8).reshape(-1)[: b.num_nodes * F.NODE2.itemsize].to(cuda)
            tb = b.tris.view(torch.uint8).reshape(-1)[: b.num_tris * F.TRI1.itemsize].to(cuda)
            count = (b.num_nodes, b.num_tris)
        else:
            nodes, tris = (np.ascontiguousarray(a) for a in b)
            if nodes.dtype != F.NODE2 or tris.dtype != F.TRI1:
                raise ValueError("pack_objects: (nodes NODE2, tris TRI1) arrays are needed")
            nb, tb, count = abi.to_device(nodes, dev), abi.to_device(tris, dev), (len(nodes), len(tris))
        if count[0] < 1 or count[1] < 1:
            raise ValueError("pack_objects: an object without nodes or triangles")
        parts.append((nb, tb))
        table[k]["num_nodes"], table[k]["num_tris"] = count
    table["node_offset"] = np.cumsum(table["num_nodes"]) - table["num_nodes"]
    table["tri_offset"] = np.cumsum(table["num_tris"]) - table["num_tris"]
    node_bytes, tri_bytes = int(table["num_nodes"].sum()) * F.NODE2.itemsize, int(table["num_tris"].sum()) * F.TRI1.itemsize
    start = (node_bytes + 255) // 256 * 256
    buffer = torch.zeros(start + tri_bytes, dtype=torch.uint8, device=cuda)
    nodes, tris = buffer[:node_bytes], buffer[start:]
    for row, (nb, tb) in zip(table, parts):
        nodes[int(row["node_offset"]) * F.NODE2.itemsize:][: nb.numel()] = nb
        tris[int(row["tri_offset"]) * F.TRI1.itemsize:][: tb.numel()] = tb
    return ObjectSet(buffer, nodes, tris, table, abi.to_device(table, dev), dev)


class Tlas:
    """A top-level hierarchy on the device: `nodes` (Node2) and `instances` (RodentInstance, in leaf order) as uint8 tensors, the info
    words of its build ([0] nodes [1] depth [2] flags), `depth`, and the scratch tensor for the next rebuild."""

    def __init__(self, nodes, instances, num_instances, info, scratch, dev):
        self.nodes, self.instances, self.num_instances, self.scratch, self.dev = nodes, instances, int(num_instances), scratch, dev
        self.info, self.num_nodes, self.depth = info, int(info[0]), int(info[1])

    @property
    def device_bytes(self):
        return self.num_nodes * F.NODE2.itemsize + self.num_instances * F.INSTANCE.itemsize


def _descriptors(transforms, object_ids, instance_ids, cuda):
    """The RodentInstanceDesc array on the device: (n, 16) int32 words."""
    t = transforms if isinstance(transforms, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(transforms, np.float32))
    n = t.shape[0] if t.dim() else 0
    if not 1 <= n <= MAX_INSTANCES:
        raise BuildError(f"num_instances = {n}: outside [1, 2^22]")
    if t.numel() != 12 * n:
        raise ValueError(f"expected (n, 12) or (n, 3, 4) transforms, got shape {tuple(t.shape)}")
    t = t.to(device=cuda, dtype=torch.float32).reshape(n, 12).contiguous()
    # Ids that come from the host are checked there; ids that are tensors already are taken as they are, with no copy back to the host
    # (the per-frame path): the instance stage keeps the low 31 bits of an instance id and checks every object id itself.
    words = []
    for name, ids in (("object_ids", object_ids), ("instance_ids", instance_ids)):
        if ids is None:
            ids = torch.arange(n, dtype=torch.int32, device=cuda)
        elif not isinstance(ids, torch.Tensor):
            ids = np.ascontiguousarray(ids).astype(np.int64)
            if name == "instance_ids" and ids.size and (ids.min() < 0 or ids.max() >= 1 << 31):
                raise BuildError("instance_ids outside [0, 2^31)")
            # (an object id past int32 becomes -1, which is outside every table too)
            ids = torch.from_numpy(np.clip(ids, -1, (1 << 31) - 1).astype(np.int32))
        if ids.shape != (n,):
            raise ValueError(f"{name}: expected {n} ids, got shape {tuple(ids.shape)}")
        words.append(ids.to(device=cuda, dtype=torch.int32))
    desc = torch.zeros((n, 16), dtype=torch.int32, device=cuda)
    desc[:, :12] = t.view(torch.int32)
    desc[:, 12], desc[:, 13] = words
    return desc


def build_tlas(objects: ObjectSet, transforms, object_ids, instance_ids=None, max_leaf=1, stream=None, scratch=None, out=None) -> Tlas:
    """Builds the top-level hierarchy over the instances (object_ids[k] placed by transforms[k], object_to_world, 3 x 4 row-major;
    instance_ids default to 0 ... n - 1) on `stream` (torch stream, None = the current one).  Raises BuildError on invalid arguments and
    on the device's flags (an object index outside the table, a singular or non-finite transform).

    scratch / out: reuse the scratch tensor / the node and instance tensors of an earlier Tlas (`out` is rebuilt in place and returned:
    the per-frame path when transforms change); they must be large enough."""
    _need_gpu()
    dev, cuda = objects.dev, f"cuda:{objects.dev}"
    if not 1 <= max_leaf <= MAX_LEAF:
        raise BuildError(f"max_leaf = {max_leaf}: outside [1, 8]")
    desc = _descriptors(transforms, object_ids, instance_ids, cuda)
    n = desc.shape[0]
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    need = abi.lib().rodent_hip_tlas_scratch_bytes(n)
    if scratch is None and out is not None:
        scratch = out.scratch
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    node_bytes, inst_bytes = max(1, n - 1) * F.NODE2.itemsize, n * F.INSTANCE.itemsize
    if out is None:
        nodes = torch.empty(node_bytes, dtype=torch.uint8, device=cuda)
        instances = torch.empty(inst_bytes, dtype=torch.uint8, device=cuda)
    else:
        nodes, instances = out.nodes, out.instances
        if nodes.numel() < node_bytes or instances.numel() < inst_bytes:
            raise ValueError("build_tlas: the buffers of `out` are too small for these instances")
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    entry = "rodent_hip_build_tlas"
    # (the counts were checked above, so the entry's own refusals of them cannot occur here)
    words = _enqueue(entry, dev, stream, info, (objects.buffer, objects.table_dev, desc, scratch, nodes, instances),
                     objects.nodes.data_ptr(), objects.table_dev.data_ptr(), objects.num_objects, desc.data_ptr(), n, int(max_leaf),
                     nodes.data_ptr(), instances.data_ptr(), scratch.data_ptr())
    if words[2]:
        raise BuildError(f"{entry}: " + ", ".join(s for bit, s in _TLAS_FLAGS if words[2] & bit))
    if out is None:
        return Tlas(nodes, instances, n, words.copy(), scratch, dev)
    out.num_instances, out.scratch = n, scratch
    out.info, out.num_nodes, out.depth = words.copy(), int(words[0]), int(words[1])
    return out


def trace_async(objects: ObjectSet, tlas: Tlas, rays_dev, hits_dev, instances_dev, num_rays, any_hit=False, stream=None):
    """Enqueues one instanced traversal pass on `stream` (torch stream or None = the current one): tensors of Ray1 in, Hit1 and (may
    be None) one int32 instance id per ray out.  A stack overflow is reported by abi.check_errors(dev, stream)."""
    if stream is None:
        stream = torch.cuda.current_stream(objects.dev)
    abi.lib().hip_traverse_instanced_bvh2_tri1_async(
        objects.dev, tlas.nodes.data_ptr(), tlas.instances.data_ptr(), objects.nodes.data_ptr(), objects.tris.data_ptr(),
        rays_dev.data_ptr(), hits_dev.data_ptr(), None if instances_dev is None else instances_dev.data_ptr(), int(num_rays),
        int(any_hit), C.c_void_p(stream.cuda_stream))


def trace(objects: ObjectSet, tlas: Tlas, rays: np.ndarray, any_hit=False):
    """Synchronous convenience wrapper: host rays in, (Hit1 array, int32 instance ids) out.  tri_id is the hit object's own prim id; a
    miss is tri_id -1, instance -1."""
    _need_gpu()
    dev, n = objects.dev, len(rays)
    rays_dev = abi.to_device(rays, dev)
    hits_dev = torch.zeros(max(n, 1) * F.HIT1.itemsize, dtype=torch.uint8, device=f"cuda:{dev}")
    ids_dev = torch.zeros(max(n, 1), dtype=torch.int32, device=f"cuda:{dev}")
    torch.cuda.synchronize(dev)
    fn = abi.lib().hip_occluded_instanced_bvh2_tri1 if any_hit else abi.lib().hip_intersect_instanced_bvh2_tri1
    fn(dev, tlas.nodes.data_ptr(), tlas.instances.data_ptr(), objects.nodes.data_ptr(), objects.tris.data_ptr(), rays_dev.data_ptr(),
       hits_dev.data_ptr(), ids_dev.data_ptr(), n)
    return abi.from_device(hits_dev, F.HIT1)[:n], ids_dev.cpu().numpy()[:n]


def download(tlas: Tlas):
    """(nodes NODE2, instances INSTANCE) host copies of a Tlas."""
    nodes = tlas.nodes[: tlas.num_nodes * F.NODE2.itemsize].cpu().numpy().view(F.NODE2).copy()
    instances = tlas.instances[: tlas.num_instances * F.INSTANCE.itemsize].cpu().numpy().view(F.INSTANCE).copy()
    return nodes, instances


# ---- moving instances: two placements per instance, a time per ray (the section "moving instances" of rodent_instances.h) -------------
class MotionTlas(Tlas):
    """A Tlas over moving instances: `instances` holds RodentMotionInstance records (both placements, in leaf order), the nodes bound
    every placement with a time in [0, 1]."""

    @property
    def device_bytes(self):
        return self.num_nodes * F.NODE2.itemsize + self.num_instances * F.MOTION_INSTANCE.itemsize


def build_motion_tlas(objects, transforms0, transforms1, object_ids, instance_ids=None, max_leaf=1, stream=None, scratch=None,
                      out=None) -> MotionTlas:
    """build_tlas for instances that move: object_ids[k] is placed by transforms0[k] at time 0 and by transforms1[k] at time 1 (both
    object_to_world, 3 x 4 row-major; tensors on the device are taken without a host copy), and linearly between them, entry by entry.
    Raises BuildError on invalid arguments and on the device's flags (an object index outside the table, a singular or non-finite
    transform at either end).  scratch / out: as in build_tlas; `out` (a MotionTlas) is rebuilt in place and returned.
    `objects`: an ObjectSet, or a MotionObjectSet (build_motion_objects): then every object's box is the union over its two keys."""
    _need_gpu()
    dev, cuda = objects.dev, f"cuda:{objects.dev}"
    if not 1 <= max_leaf <= MAX_LEAF:
        raise BuildError(f"max_leaf = {max_leaf}: outside [1, 8]")
    first = _descriptors(transforms0, object_ids, instance_ids, cuda)
    n = first.shape[0]
    t1 = transforms1 if isinstance(transforms1, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(transforms1, np.float32))
    if t1.numel() != 12 * n:
        raise ValueError(f"expected {n} (12,) or (3, 4) transforms at time 1, got shape {tuple(t1.shape)}")
    desc = torch.zeros((n, 32), dtype=torch.int32, device=cuda)
    desc[:, :12] = first[:, :12]
    desc[:, 12:24] = t1.to(device=cuda, dtype=torch.float32).reshape(n, 12).contiguous().view(torch.int32)
    desc[:, 24:26] = first[:, 12:14]
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    need = abi.lib().rodent_hip_motion_tlas_scratch_bytes(n)
    if scratch is None and out is not None:
        scratch = out.scratch
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    node_bytes, inst_bytes = max(1, n - 1) * F.NODE2.itemsize, n * F.MOTION_INSTANCE.itemsize
    if out is None:
        nodes = torch.empty(node_bytes, dtype=torch.uint8, device=cuda)
        instances = torch.empty(inst_bytes, dtype=torch.uint8, device=cuda)
    else:
        nodes, instances = out.nodes, out.instances
        if nodes.numel() < node_bytes or instances.numel() < inst_bytes:
            raise ValueError("build_motion_tlas: the buffers of `out` are too small for these instances")
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    entry = "rodent_hip_build_motion_tlas" + ("_motion_objects" if isinstance(objects, MotionObjectSet) else "")
    words = _enqueue(entry, dev, stream, info, (objects.buffer, objects.table_dev, desc, scratch, nodes, instances),
                     objects.nodes.data_ptr(), objects.table_dev.data_ptr(), objects.num_objects, desc.data_ptr(), n, int(max_leaf),
                     nodes.data_ptr(), instances.data_ptr(), scratch.data_ptr())
    if words[2]:
        raise BuildError(f"{entry}: " + ", ".join(s for bit, s in _TLAS_FLAGS if words[2] & bit))
    if out is None:
        return MotionTlas(nodes, instances, n, words.copy(), scratch, dev)
    out.num_instances, out.scratch = n, scratch
    out.info, out.num_nodes, out.depth = words.copy(), int(words[0]), int(words[1])
    return out


def trace_motion_async(objects, tlas: MotionTlas, rays_dev, times_dev, hits_dev, instances_dev, num_rays, any_hit=False,
                       stream=None):
    """trace_async through a MotionTlas: `times_dev` holds one float32 per ray, the time at which that ray sees every instance -- and,
    with a MotionObjectSet, every object; a ray whose time is not in [0, 1] is then a miss."""
    if stream is None:
        stream = torch.cuda.current_stream(objects.dev)
    l = abi.lib()
    fn = (l.hip_traverse_motion_instanced_motion_bvh2_tri1_async if isinstance(objects, MotionObjectSet)
          else l.hip_traverse_motion_instanced_bvh2_tri1_async)
    fn(
        objects.dev, tlas.nodes.data_ptr(), tlas.instances.data_ptr(), objects.nodes.data_ptr(), objects.tris.data_ptr(),
        rays_dev.data_ptr(), times_dev.data_ptr(), hits_dev.data_ptr(), None if instances_dev is None else instances_dev.data_ptr(),
        int(num_rays), int(any_hit), C.c_void_p(stream.cuda_stream))


def trace_motion(objects, tlas: MotionTlas, rays: np.ndarray, times, any_hit=False):
    """Synchronous convenience wrapper: host rays and their times (one float32 each) in, (Hit1 array, int32 instance ids) out."""
    _need_gpu()
    dev, n = objects.dev, len(rays)
    times = np.ascontiguousarray(times, np.float32)
    if times.shape != (n,):
        raise ValueError(f"trace_motion: expected {n} times, got shape {times.shape}")
    rays_dev = abi.to_device(rays, dev)
    times_dev = torch.from_numpy(times if n else np.zeros(1, np.float32)).to(f"cuda:{dev}")
    hits_dev = torch.zeros(max(n, 1) * F.HIT1.itemsize, dtype=torch.uint8, device=f"cuda:{dev}")
    ids_dev = torch.zeros(max(n, 1), dtype=torch.int32, device=f"cuda:{dev}")
    torch.cuda.synchronize(dev)
    kind = "motion_instanced_motion_bvh2_tri1" if isinstance(objects, MotionObjectSet) else "motion_instanced_bvh2_tri1"
    fn = getattr(abi.lib(), ("hip_occluded_" if any_hit else "hip_intersect_") + kind)
    fn(dev, tlas.nodes.data_ptr(), tlas.instances.data_ptr(), objects.nodes.data_ptr(), objects.tris.data_ptr(), rays_dev.data_ptr(),
       times_dev.data_ptr(), hits_dev.data_ptr(), ids_dev.data_ptr(), n)
    return abi.from_device(hits_dev, F.HIT1)[:n], ids_dev.cpu().numpy()[:n]


def download_motion(tlas: MotionTlas):
    """(nodes NODE2, instances MOTION_INSTANCE) host copies of a MotionTlas."""
    nodes = tlas.nodes[: tlas.num_nodes * F.NODE2.itemsize].cpu().numpy().view(F.NODE2).copy()
    instances = tlas.instances[: tlas.num_instances * F.MOTION_INSTANCE.itemsize].cpu().numpy().view(F.MOTION_INSTANCE).copy()
    return nodes, instances


# ---- deforming objects: the listed objects of an ObjectSet refitted in place, in one launch list (rodent_hip_refit_objects) ----------
class RefitPlan:
    """What refit_objects needs of a list of objects, prepared once: the RodentRefitRange table on the host (`table`,
    formats.REFIT_RANGE) and on the device (`table_dev`), the listed objects' node and record totals and the scratch bytes."""

    def __init__(self, table, table_dev, num_nodes, num_recs, scratch_bytes):
        self.table, self.table_dev, self.num_listed = table, table_dev, len(table)
        self.num_nodes, self.num_recs, self.scratch_bytes = int(num_nodes), int(num_recs), int(scratch_bytes)


def plan_refit(objects: ObjectSet, object_ids, ranges) -> RefitPlan:
    """The plan of refit_objects for the objects `object_ids` (any order) of `objects`; `ranges`: one (first_tri, num_tris) row per
    listed object, its rows of the concatenated index table (rodent_hip_refit_objects_plan).  An id outside the table is kept: the
    device flags it."""
    ids = np.ascontiguousarray(np.clip(np.asarray(object_ids, np.int64).reshape(-1), -1, (1 << 31) - 1).astype(np.int32))
    rows = np.asarray(ranges, np.int32).reshape(-1, 2)
    if len(ids) < 1 or len(rows) != len(ids):
        raise ValueError(f"plan_refit: {len(ids)} object ids and {len(rows)} (first_tri, num_tris) rows")
    first, count = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    table, totals = np.zeros(len(ids), F.REFIT_RANGE), np.zeros(2, np.int32)
    host = np.ascontiguousarray(objects.table)
    need = abi.lib().rodent_hip_refit_objects_plan(host.ctypes.data, len(host), ids.ctypes.data, first.ctypes.data, count.ctypes.data,
                                                   len(ids), table.ctypes.data, totals.ctypes.data)
    if need < 0:
        raise BuildError("rodent_hip_refit_objects_plan: the listed objects hold more than 2^31 - 1 nodes or records")
    return RefitPlan(table, abi.to_device(table, objects.dev), totals[0], totals[1], need)


def refit_objects(objects: ObjectSet, object_ids, vertices, indices, ranges, stream=None, scratch=None, check=True):
    """Refits the objects `object_ids` of `objects` in place to moved `vertices` (rodent_hip_refit_objects): new boxes and Tri1 records
    for the listed objects, the same topologies, every other object's bytes as they are.  `vertices` and `indices` are the concatenated
    tables of all objects ((n, 3) or (n, 4); tensors on the device are not copied); `ranges` is one (first_tri, num_tris) row per listed
    object, or a RefitPlan of plan_refit (then `object_ids` is not read and nothing is uploaded).  The launch list does not grow with
    the list.  Returns the info words ([0] nodes completed over the listed objects, [1] records rewritten, [2] flags); with `check` it
    raises BuildError on a flag and when a node stayed incomplete.  scratch: a uint8 tensor to reuse, large enough."""
    _need_gpu()
    from .gpubuild import _columns4
    dev, cuda = objects.dev, f"cuda:{objects.dev}"
    plan = ranges if isinstance(ranges, RefitPlan) else plan_refit(objects, object_ids, ranges)
    v, ix = _columns4(vertices, torch.float32, dev), _columns4(indices, torch.int32, dev)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    if scratch is None or scratch.numel() * scratch.element_size() < plan.scratch_bytes:
        scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=cuda)
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    entry = "rodent_hip_refit_objects"
    words = _enqueue(entry, dev, stream, info, (v, ix, scratch, objects.buffer, objects.table_dev, plan.table_dev), v.data_ptr(),
                     v.shape[0], ix.data_ptr(), ix.shape[0], objects.nodes.data_ptr(), objects.tris.data_ptr(),
                     objects.table_dev.data_ptr(), objects.num_objects, plan.table_dev.data_ptr(), plan.num_listed, plan.num_nodes,
                     plan.num_recs, scratch.data_ptr()).copy()
    if check and words[2]:
        raise BuildError(f"{entry}: " + ", ".join(s for bit, s in _TLAS_FLAGS if words[2] & bit))
    if check and words[0] != plan.num_nodes:
        raise BuildError(f"{entry}: malformed hierarchy ({words[0]} of {plan.num_nodes} nodes completed)")
    return words


# ---- deforming objects under moving instances: two-key records for every object of a set (rodent_hip_build_motion_objects) ----------
class MotionObjectSet:
    """The packed motion objects: every object's RodentMotionNode2 records in `nodes`, every object's RodentMotionTri1 records in `tris`
    (uint8 views of ONE allocation, `buffer`), and the RodentObject table, whose offsets count motion records: it is the table of the
    ObjectSet the records were built over.  `info`: the words of the build, `scratch` its scratch tensor."""

    def __init__(self, buffer, nodes, tris, table, table_dev, dev, info=None, scratch=None):
        self.buffer, self.nodes, self.tris, self.table, self.table_dev, self.dev = buffer, nodes, tris, table, table_dev, dev
        self.num_objects, self.num_nodes, self.num_tris = len(table), int(table["num_nodes"].sum()), int(table["num_tris"].sum())
        self.info, self.scratch = info, scratch

    @property
    def device_bytes(self):
        return self.buffer.numel() + self.table_dev.numel() * self.table_dev.element_size()


def _motion_room(num_nodes, num_recs, cuda):
    node_bytes = num_nodes * F.MOTION_NODE2.itemsize
    start = (node_bytes + 255) // 256 * 256
    buffer = torch.zeros(start + num_recs * F.MOTION_TRI1.itemsize, dtype=torch.uint8, device=cuda)
    return buffer, buffer[:node_bytes], buffer[start:]


def build_motion_objects(objects: ObjectSet, vertices0, vertices1, indices, ranges, stream=None, scratch=None, out=None,
                         check=True) -> MotionObjectSet:
    """The two-key records of ALL objects of `objects` (the topologies; only read) over `vertices0` at time 0 and `vertices1` at time 1, in
    one launch list whatever their number (rodent_hip_build_motion_objects).  `vertices*` and `indices` are the concatenated tables of
    all objects ((n, 3) or (n, 4); tensors on the device are not copied); `ranges`: one (first_tri, num_tris) row per object, in table
    order, or a RefitPlan of plan_refit over all objects.  Per object the records are those motion.build_motion_bvh2 writes for it alone.
    scratch / out: reuse the scratch tensor / the record tensors of an earlier result: `out=` is the refit to moved keys, in place.
    info: [0] nodes completed at key 0 [1] records fused [2] flags [3] nodes completed at key 1.  With `check` a flag or an incomplete
    key raises BuildError."""
    _need_gpu()
    from .gpubuild import _columns4
    dev, cuda = objects.dev, f"cuda:{objects.dev}"
    plan = ranges if isinstance(ranges, RefitPlan) else plan_refit(objects, np.arange(objects.num_objects), ranges)
    if plan.num_listed != objects.num_objects or not np.array_equal(plan.table["object"], np.arange(objects.num_objects)):
        raise ValueError("build_motion_objects: one range per object, in table order, is needed")
    v0, v1, ix = _columns4(vertices0, torch.float32, dev), _columns4(vertices1, torch.float32, dev), _columns4(indices, torch.int32, dev)
    if v0.shape[0] != v1.shape[0]:
        raise ValueError(f"build_motion_objects: {v0.shape[0]} vertices at time 0, {v1.shape[0]} at time 1")
    num_nodes, num_recs = objects.nodes.numel() // F.NODE2.itemsize, objects.tris.numel() // F.TRI1.itemsize
    if out is None:
        buffer, nodes, tris = _motion_room(num_nodes, num_recs, cuda)
    else:
        buffer, nodes, tris = out.buffer, out.nodes, out.tris
        if nodes.numel() < num_nodes * F.MOTION_NODE2.itemsize or tris.numel() < num_recs * F.MOTION_TRI1.itemsize:
            raise ValueError("build_motion_objects: the buffers of `out` are too small for this set")
    entry = "rodent_hip_build_motion_objects"
    need = abi.lib().rodent_hip_motion_objects_scratch_bytes(num_nodes, num_recs, plan.scratch_bytes)
    if need < 0:
        raise BuildError(f"{entry}: an object set without nodes or records")
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    if scratch is None and out is not None:
        scratch = out.scratch
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    words = _enqueue(entry, dev, stream, info, (v0, v1, ix, scratch, objects.buffer, objects.table_dev, plan.table_dev, buffer),
                     v0.data_ptr(), v1.data_ptr(), v0.shape[0], ix.data_ptr(), ix.shape[0], objects.nodes.data_ptr(), num_nodes,
                     objects.tris.data_ptr(), num_recs, objects.table_dev.data_ptr(), objects.num_objects, plan.table_dev.data_ptr(),
                     plan.num_listed, plan.num_nodes, plan.num_recs, nodes.data_ptr(), tris.data_ptr(), scratch.data_ptr()).copy()
    if out is None:
        out = MotionObjectSet(buffer, nodes, tris, objects.table.copy(), objects.table_dev, dev)
    out.info, out.scratch = words, scratch
    if check and words[2]:
        raise BuildError(f"{entry}: " + ", ".join(s for bit, s in _TLAS_FLAGS if words[2] & bit))
    if check and (words[0] != plan.num_nodes or words[3] != plan.num_nodes):
        raise BuildError(f"{entry}: malformed hierarchy ({words[0]} and {words[3]} of {plan.num_nodes} nodes completed)")
    return out


def pack_motion_objects(mbvhs, dev=0) -> MotionObjectSet:
    """Packs motion.MotionBvh objects or (nodes MOTION_NODE2, tris MOTION_TRI1) numpy pairs into one MotionObjectSet: concatenation, no
    id is rewritten."""
    _need_gpu()
    if not len(mbvhs):
        raise ValueError("pack_motion_objects: at least one object is needed")
    cuda = f"cuda:{dev}"
    parts, table = [], np.zeros(len(mbvhs), F.OBJECT)
    for k, b in enumerate(mbvhs):
        if isinstance(b, tuple):
            nodes, tris = (np.ascontiguousarray(a) for a in b)
            if nodes.dtype != F.MOTION_NODE2 or tris.dtype != F.MOTION_TRI1:
                raise ValueError("pack_motion_objects: (nodes MOTION_NODE2, tris MOTION_TRI1) arrays are needed")
            nb, tb, count = abi.to_device(nodes, dev), abi.to_device(tris, dev), (len(nodes), len(tris))
        else:
            nb = b.nodes.view(torch.uint8).reshape(-1)[: b.num_nodes * F.MOTION_NODE2.itemsize].to(cuda)
            tb = b.tris.view(torch.uint8).reshape(-1)[: b.num_tris * F.MOTION_TRI1.itemsize].to(cuda)
            count = (b.num_nodes, b.num_tris)
        if count[0] < 1 or count[1] < 1:
            raise ValueError("pack_motion_objects: an object without nodes or triangles")
        parts.append((nb, tb))
        table[k]["num_nodes"], table[k]["num_tris"] = count
    table["node_offset"] = np.cumsum(table["num_nodes"]) - table["num_nodes"]
    table["tri_offset"] = np.cumsum(table["num_tris"]) - table["num_tris"]
    buffer, nodes, tris = _motion_room(int(table["num_nodes"].sum()), int(table["num_tris"].sum()), cuda)
    for row, (nb, tb) in zip(table, parts):
        nodes[int(row["node_offset"]) * F.MOTION_NODE2.itemsize:][: nb.numel()] = nb
        tris[int(row["tri_offset"]) * F.MOTION_TRI1.itemsize:][: tb.numel()] = tb
    return MotionObjectSet(buffer, nodes, tris, table, abi.to_device(table, dev), dev)


def download_motion_objects(objects: MotionObjectSet):
    """(nodes MOTION_NODE2, tris MOTION_TRI1) host copies of the packed records, the whole arrays."""
    return (objects.nodes.cpu().numpy().view(F.MOTION_NODE2).copy(), objects.tris.cpu().numpy().view(F.MOTION_TRI1).copy())


# ---- the objects' hierarchies built in one launch list (rodent_hip_build_objects: csrc/build_forest.h) ----------------------------
def _build_plan(object_ids, ranges, dev):
    """(RodentRefitRange table on the host, on the device, listed triangles, scratch bytes) of rodent_hip_build_objects_plan."""
    ids = np.ascontiguousarray(np.clip(np.asarray(object_ids, np.int64).reshape(-1), -1, (1 << 31) - 1).astype(np.int32))
    rows = np.asarray(ranges, np.int32).reshape(-1, 2)
    if len(ids) < 1 or len(rows) != len(ids):
        raise ValueError(f"{len(ids)} object ids and {len(rows)} (first_tri, num_tris) rows")
    first, count = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    table, totals = np.zeros(len(ids), F.REFIT_RANGE), np.zeros(2, np.int32)
    need = abi.lib().rodent_hip_build_objects_plan(ids.ctypes.data, first.ctypes.data, count.ctypes.data, len(ids), table.ctypes.data,
                                                   totals.ctypes.data)
    if need < 0:
        raise BuildError("rodent_hip_build_objects_plan: more than 2^20 objects, an object without triangles or more than 2^25 triangles")
    return table, abi.to_device(table, dev), int(totals[0]), int(need)


def _build_objects(mode, plan, vertices, indices, max_leaf, dev, stream, scratch, nodes, tris, table_dev, num_objects, keep):
    """rodent_hip_build_objects on `stream`: (info words, (K, 4) per-object info words) on the host."""
    if not 1 <= max_leaf <= MAX_LEAF:
        raise BuildError(f"max_leaf = {max_leaf}: outside [1, 8]")
    from .gpubuild import _columns4
    ranges, ranges_dev, total, need = plan
    cuda = f"cuda:{dev}"
    v, ix = _columns4(vertices, torch.float32, dev), _columns4(indices, torch.int32, dev)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    object_info = torch.empty((len(ranges), 4), dtype=torch.int32, device=cuda)
    words = _enqueue("rodent_hip_build_objects", dev, stream, info, (v, ix, scratch, ranges_dev, object_info, table_dev, *keep),
                     v.data_ptr(), v.shape[0], ix.data_ptr(), ix.shape[0], int(max_leaf), int(mode), nodes.data_ptr(), tris.data_ptr(),
                     table_dev.data_ptr(), int(num_objects), ranges_dev.data_ptr(), len(ranges), total, scratch.data_ptr(),
                     object_info.data_ptr()).copy()
    return words, object_info.cpu().numpy()


def _raise_object_flags(entry, words, per_object, ids):
    if words[2]:
        bad = np.nonzero(per_object[:, 2])[0]
        k = int(bad[0]) if len(bad) else 0
        flags = int(per_object[k, 2]) if len(bad) else int(words[2])
        raise BuildError(f"{entry}: object {int(ids[k])}: " + ", ".join(s for bit, s in _TLAS_FLAGS if flags & bit))


def build_objects(vertices, indices, ranges, max_leaf=2, dev=0, stream=None, slots=False, check=True) -> ObjectSet:
    """Builds the BVH2 / Tri1 hierarchies of ALL objects of a new set in one launch list (rodent_hip_build_objects), whatever their
    number: `vertices` and `indices` are the concatenated tables ((n, 3) or (n, 4); tensors on the device are not copied), `ranges` one
    (first_tri, num_tris) row per object.  Every object's records are those build_bvh2(vertices, indices[first: first + n], max_leaf)
    writes for it alone.  slots=False: the tight set, equal to pack_objects of the per-object builds.  slots=True: every object keeps a
    node slot of max(1, n - 1) records (`capacities`), so rebuild_objects can rebuild any of them where it lies.  `depths` holds every
    object's depth.  With `check` a device flag raises BuildError naming the first flagged object."""
    _need_gpu()
    rows = np.asarray(ranges, np.int32).reshape(-1, 2)
    ids = np.arange(len(rows), dtype=np.int32)
    plan = _build_plan(ids, rows, dev)
    total, cuda = plan[2], f"cuda:{dev}"
    room = np.maximum(rows[:, 1].astype(np.int64) - 1, 1)
    node_bytes = int(room.sum()) * F.NODE2.itemsize
    start = (node_bytes + 255) // 256 * 256
    buffer = torch.zeros(start + total * F.TRI1.itemsize, dtype=torch.uint8, device=cuda)
    table = np.zeros(len(rows), F.OBJECT)
    if slots:
        table["node_offset"], table["tri_offset"], table["num_tris"] = np.cumsum(room) - room, plan[0]["rec_start"], rows[:, 1]
    table_dev = abi.to_device(table, dev)
    entry = "rodent_hip_build_objects"
    words, per_object = _build_objects(0 if slots else 1, plan, vertices, indices, max_leaf, dev, stream, None, buffer[:node_bytes],
                                       buffer[start:], table_dev, len(rows), (buffer,))
    if check:
        _raise_object_flags(entry, words, per_object, ids)
    table = abi.from_device(table_dev, F.OBJECT).copy()
    if not slots:                                                # the nodes lie tight at the front of their room
        node_bytes = int(table["num_nodes"].sum()) * F.NODE2.itemsize
    return ObjectSet(buffer, buffer[:node_bytes], buffer[start:], table, table_dev, dev, room.astype(np.int32) if slots else None,
                     per_object[:, 1].copy())


def rebuild_objects(objects: ObjectSet, object_ids, vertices, indices, ranges, max_leaf=2, stream=None, scratch=None, check=True):
    """Rebuilds the hierarchies of the objects `object_ids` (any order) of a slotted set (build_objects(slots=True)) where they lie,
    from moved `vertices`: new topologies, not a refit.  `ranges`: one (first_tri, num_tris) row per listed object; its triangle count
    must be its slot's.  One launch list whatever the list's length; every other object keeps its bytes.  Returns (info words, per-object
    info words); with `check` the host table is refreshed (one K x 16-byte copy), `depths` updated and a flag raises BuildError naming
    the first flagged object.  Raises ValueError on a tight set or a triangle count that differs from the slot's."""
    _need_gpu()
    if objects.capacities is None:
        raise ValueError("rebuild_objects: a slotted set is needed (build_objects(slots=True))")
    ids = np.asarray(object_ids, np.int64).reshape(-1)
    rows = np.asarray(ranges, np.int32).reshape(-1, 2)
    if len(rows) != len(ids):
        raise ValueError(f"rebuild_objects: {len(ids)} object ids and {len(rows)} (first_tri, num_tris) rows")
    known = (ids >= 0) & (ids < objects.num_objects)
    if (objects.table["num_tris"][ids[known]] != rows[known, 1]).any():
        raise ValueError("rebuild_objects: a listed object's triangle count differs from its slot's")
    plan = _build_plan(ids, rows, objects.dev)
    entry = "rodent_hip_build_objects"
    words, per_object = _build_objects(0, plan, vertices, indices, max_leaf, objects.dev, stream, scratch, objects.nodes, objects.tris,
                                       objects.table_dev, objects.num_objects, (objects.buffer,))
    if check:
        objects.table = abi.from_device(objects.table_dev, F.OBJECT).copy()
        objects.num_nodes = int(objects.table["num_nodes"].sum())
        if objects.depths is not None:
            objects.depths[ids[known]] = per_object[known, 1]
        _raise_object_flags(entry, words, per_object, ids)
    return words, per_object


# ---- instanced scenes for the renderer (include/rodent_render.h: rodent_hip_scene_create_instanced; render.Renderer(instances=...)) ----
class ObjectScene:
    """The concatenated tables of several scene.Scene objects, in object space, duck-typed like scene.Scene (no hierarchy: the
    renderer builds every object's on the device), and `ranges`: (num_objects, 4) int32 rows first_tri, num_tris, first_light,
    num_lights."""

    @property
    def num_tris(self):
        return len(self.indices)


def concat_scenes(scenes) -> ObjectScene:
    """Concatenates scene.Scene objects into the one description an instanced scene is created from: vertex ids, material ids, texture
    ids, texel offsets and the light ids of emissive triangles are offset by what lies in front of them (a triangle that does not emit
    keeps light id 0), so every object keeps its own materials, textures and lights."""
    from .scene import LIGHT, MATERIAL, TEXTURE
    if not len(scenes):
        raise ValueError("concat_scenes: at least one object is needed")
    out = ObjectScene()
    parts = {n: [] for n in ("vertices", "normals", "face_normals", "indices", "materials", "lights", "light_ids", "texcoords",
                             "textures", "texels")}
    ranges = np.zeros((len(scenes), 4), np.int32)
    nv = nt = nm = nl = ntex = ntexel = 0
    for k, s in enumerate(scenes):
        ind = np.array(s.indices, np.int32).reshape(-1, 4)
        emissive = np.asarray(s.materials)["emissive"][ind[:, 3]] != 0
        ranges[k] = (nt, len(ind), nl, len(s.lights))
        ind[:, :3] += nv; ind[:, 3] += nm
        mats = np.array(s.materials, MATERIAL)
        for f in ("tex_kd", "tex_ks"):
            mats[f] = np.where(mats[f] > 0, mats[f] + ntex, 0)
        tex = np.array(s.textures, TEXTURE)
        tex["offset"] += np.uint32(ntexel)
        for n, a in (("vertices", s.vertices), ("normals", s.normals), ("face_normals", s.face_normals), ("indices", ind),
                     ("materials", mats), ("lights", np.asarray(s.lights, LIGHT)),
                     ("light_ids", np.where(emissive, np.asarray(s.light_ids, np.int32) + nl, 0).astype(np.int32)),
                     ("texcoords", s.texcoords), ("textures", tex), ("texels", np.asarray(s.texels, np.uint32))):
            parts[n].append(a)
        nv += len(s.vertices); nt += len(ind); nm += len(mats); nl += len(s.lights); ntex += len(tex); ntexel += len(s.texels)
    for n, p in parts.items():
        setattr(out, n, np.ascontiguousarray(np.concatenate(p)))
    out.nodes, out.tris = np.zeros(0, F.NODE2), np.zeros(0, F.TRI1)
    out.ranges = ranges
    return out
