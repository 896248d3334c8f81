"""Instanced scenes on the GPU (include/rodent_instances.h; rodent_amd/instances.py) against tests/instance_model.py.

* the TLAS's nodes, instance records and info words equal the model's byte for byte, on any stream, into reused scratch and outputs;
* hit records and instance ids equal the model's exactly: two objects, 9 overlapping instances, camera rays and segments, whole and cut
  to 1 / 63 / 64 / 65 rays, closest and any-hit, with and without the instance-id array;
* one identity instance of a reference-built hierarchy gives the shipped BVH2 kernel's hit records;
* a hand-made TLAS (one leaf of three instances beside an empty slot);
* the stack: P + 2 == 64 is traced, a deeper object raises the flag and the next launch is clean;
* transforms moved and the TLAS rebuilt in place on another stream;
* refused arguments and the two device flags.
"""
import ctypes as C
import gzip

import numpy as np
import pytest

import instance_model as M
from conftest import GOLDEN, chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 63, 64, 65, 257, 1000)
IDENTITY = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
MOVED_RAYS = 1722          # of the 2048 rays of test_moved_transforms, those whose record the move changes (the model's count)


@pytest.fixture(scope="module")
def gi(native_build):
    import torch
    from rodent_amd import instances
    assert torch.cuda.is_available(), "these tests need a GPU"
    return instances


@pytest.fixture(scope="module")
def two_objects(gi, cornell):
    """The Cornell block and the flat quad, packed on the device and in the model."""
    pairs = [cornell.blocks[2], M.flat_object()]
    return gi.pack_objects(pairs), M.pack(pairs)


def small_soup(n, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), np.float32)
    centre = rng.uniform(-1, 1, (n, 1, 3))
    v[:, :3] = (centre + rng.uniform(-0.3, 0.3, (n, 3, 3))).reshape(3 * n, 3).astype(np.float32)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


def same_tlas(gi, tlas, model):
    nodes, inst = gi.download(tlas)
    m_nodes, m_inst, m_info = model
    assert np.array_equal(tlas.info, m_info), (tlas.info, m_info)
    assert nodes.tobytes() == m_nodes.tobytes() and inst.tobytes() == m_inst.tobytes()


@pytest.mark.parametrize("max_leaf", [1, 2, 8])
def test_tlas_bytes_equal_the_model(gi, two_objects, max_leaf):
    objects, (p_nodes, _, table) = two_objects
    for n in SIZES:
        transforms, obj = M.seeded_transforms(n, 100 * max_leaf + n, 40.0, 2)
        assert n < 3 or (np.linalg.det(transforms.reshape(n, 3, 4)[:, :, :3].astype(np.float64)) < 0).any()      # a mirror
        ids = (np.arange(n) * 7 + 5).astype(np.int64)
        model = M.build_tlas(p_nodes, table, M.descriptors(transforms, obj, ids), max_leaf)
        assert model[2][2] == 0
        same_tlas(gi, gi.build_tlas(objects, transforms, obj, ids, max_leaf), model)


def test_tlas_on_two_streams_and_into_reused_buffers(gi, two_objects):
    import torch
    objects, (p_nodes, _, table) = two_objects
    transforms, obj = M.seeded_transforms(1000, 9, 40.0, 2)
    model = M.build_tlas(p_nodes, table, M.descriptors(transforms, obj), 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = gi.build_tlas(objects, transforms, obj, max_leaf=2, stream=s1)
    b = gi.build_tlas(objects, transforms, obj, max_leaf=2, stream=s2)
    same_tlas(gi, a, model); same_tlas(gi, b, model)
    # the scratch and the outputs of another, larger build (their contents are that build's), then this one into them
    t2, o2 = M.seeded_transforms(5000, 10, 40.0, 2)
    big = gi.build_tlas(objects, t2, o2, max_leaf=1)
    ptrs = (big.nodes.data_ptr(), big.instances.data_ptr(), big.scratch.data_ptr())
    c = gi.build_tlas(objects, transforms, obj, max_leaf=2, scratch=big.scratch, out=big)
    assert c is big and ptrs == (c.nodes.data_ptr(), c.instances.data_ptr(), c.scratch.data_ptr())
    same_tlas(gi, c, model)


# ---- trace parity ---------------------------------------------------------------------------------------------------------------
def parity_layout(seed=21):
    """9 instances of two objects crowded around the Cornell box's place: an identity, mirrors (every third), a coincident pair
    (0 and 1), boxes that overlap each other."""
    transforms, obj = M.seeded_transforms(9, seed, 1.2, 2)
    transforms[3], obj[3] = IDENTITY, 0
    return transforms, obj, (np.arange(9) * 11 + 3).astype(np.int64)


def scene_rays(cornell, count, seed):
    rng = np.random.default_rng(seed)
    a, b = (rng.uniform(-4, 4, (count, 3)).astype(np.float32) for _ in range(2))
    return {"camera": cornell.ray_sets["primary"], "segments": F.make_rays(a, b - a, 0.0, 1.0)}


@pytest.fixture(scope="module")
def parity(gi, oracle, cornell):
    """Objects (the Cornell block, a device-built soup of 300 triangles), the TLAS on both sides, the rays, the model's answers."""
    from rodent_amd import gpubuild
    soup = gpubuild.build_bvh2(*small_soup(300, 4), max_leaf=2)
    objects = gi.pack_objects([abi_bvh(cornell), soup])
    p_nodes, p_tris, table = M.pack([cornell.blocks[2], gpubuild.download(soup)])
    transforms, obj, ids = parity_layout()
    model = M.build_tlas(p_nodes, table, M.descriptors(transforms, obj, ids), 1)
    tlas = gi.build_tlas(objects, transforms, obj, ids, 1)
    same_tlas(gi, tlas, model)
    rays = scene_rays(cornell, 4096, 8)
    expect = {(name, any_hit): M.trace(oracle, model[0], model[1], p_nodes, p_tris, r, any_hit)
              for name, r in rays.items() for any_hit in (False, True)}
    return objects, tlas, rays, expect, (p_nodes, p_tris, table)


def abi_bvh(cornell):
    from rodent_amd import abi
    return abi.DeviceBvh(2, *cornell.blocks[2], 0)


@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name", ["camera", "segments"])
def test_trace_equals_the_model(gi, parity, name, any_hit):
    import torch
    from rodent_amd import abi
    objects, tlas, rays, expect, _ = parity
    m_hits, m_ids = expect[(name, any_hit)]
    share = (m_hits["tri_id"] >= 0).mean()
    print(f"{name} any_hit={any_hit}: hit share {share:.3f}, instances hit {sorted(set(m_ids[m_ids >= 0]))}")
    assert share > 0.05 and len(set(m_ids[m_ids >= 0])) >= 3
    for count in (len(rays[name]), 1, 63, 64, 65):
        hits, ids = gi.trace(objects, tlas, rays[name][:count], any_hit)
        assert hits.tobytes() == m_hits[:count].tobytes(), (name, any_hit, count)
        assert np.array_equal(ids, m_ids[:count]), (name, any_hit, count)
        # without the instance-id array: the same hit records
        rays_dev = abi.to_device(rays[name][:count])
        hits_dev = torch.zeros(count * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        gi.trace_async(objects, tlas, rays_dev, hits_dev, None, count, any_hit)
        abi.check_errors(0)
        assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits[:count].tobytes()


def test_identity_instance_against_the_shipped_kernel(gi, tmp_path):
    from rodent_amd import abi, raygen
    path = tmp_path / "atrium.bvh"
    path.write_bytes(gzip.decompress((GOLDEN / "atrium-decimated-refbuilt.bvh.gz").read_bytes()))
    nodes, tris = F.read_bvh(path, F.BVH2_TRI1)
    bvh = abi.DeviceBvh(2, nodes, tris, 0)
    objects = gi.pack_objects([bvh])
    tlas = gi.build_tlas(objects, IDENTITY[None], [0], [0])
    lo, hi = raygen.scene_bounds2(nodes)
    rays = np.concatenate([raygen.random_rays(lo, hi, 20000, 3, 0.0, 1.0), raygen.random_rays(lo, hi, 20000, 4, 0.0, 5000.0)])
    # the decimated atrium is mostly air: every second ray is aimed at a point of a triangle, so the long ones among them (a quarter of
    # all rays) pass through the scene's surface and the shares compared below are not shares of misses
    rng = np.random.default_rng(5)
    t = tris[rng.integers(0, len(tris), len(rays) // 2)]
    w = rng.dirichlet([1, 1, 1], len(t)).astype(np.float32)
    target = w[:, :1] * t["v0"] + w[:, 1:2] * (t["v0"] - t["e1"]) + w[:, 2:] * (t["v0"] + t["e2"])
    rays["dir"][::2] = target - rays["org"][::2]
    for any_hit in (False, True):
        ref = abi.traverse(bvh, rays, any_hit=any_hit)
        hits, ids = gi.trace(objects, tlas, rays, any_hit)
        assert hits.tobytes() == ref.tobytes()
        assert np.array_equal(ids, np.where(ref["tri_id"] >= 0, 0, -1)) and (ref["tri_id"] >= 0).mean() > 0.2


def upload_tlas(gi, nodes, inst):
    from rodent_amd import abi
    return gi.Tlas(abi.to_device(nodes), abi.to_device(inst), len(inst), np.int32([len(nodes), 1, 0, 0]), None, 0)


def test_hand_made_tlas(gi, oracle, parity, cornell):
    """One node: a leaf of three instances (the sentinel on the third) beside an empty slot (child 0, bounds +inf / -inf)."""
    objects, _, rays, _, (p_nodes, p_tris, table) = parity
    transforms, obj, ids = parity_layout()
    w, bad = M.invert(transforms[[3, 0, 5]])
    assert not bad.any()
    inst = np.zeros(3, F.INSTANCE)
    inst["world_to_object"] = w
    inst["node_offset"], inst["tri_offset"] = table["node_offset"][obj[[3, 0, 5]]], table["tri_offset"][obj[[3, 0, 5]]]
    inst["instance_id"] = [40, 41, 42 | -(1 << 31)]
    node = np.zeros(1, F.NODE2)
    node["bounds"][0, :6] = [-10, 10, -10, 10, -10, 10]
    node["bounds"][0, 6::2], node["bounds"][0, 7::2] = np.inf, -np.inf
    node["child"][0] = [~0, 0]
    tlas = upload_tlas(gi, node, inst)
    for name in ("camera", "segments"):
        for any_hit in (False, True):
            m_hits, m_ids = M.trace(oracle, node, inst, p_nodes, p_tris, rays[name][:1024], any_hit)
            hits, got_ids = gi.trace(objects, tlas, rays[name][:1024], any_hit)
            assert hits.tobytes() == m_hits.tobytes() and np.array_equal(got_ids, m_ids)
            assert set(m_ids) <= {-1, 40, 41, 42} and (name == "camera" or set(m_ids) == {-1, 40, 41, 42})


# ---- stack ----------------------------------------------------------------------------------------------------------------------
def chain_scene(gi, depth, levels):
    """conftest.chain_bvh2(depth) as the one object, under an identity instance whose single-leaf TLAS is padded by `levels` nodes."""
    obj = chain_bvh2(depth)
    p_nodes, p_tris, table = M.pack([obj])
    root, inst, _ = M.build_tlas(p_nodes, table, M.descriptors(IDENTITY[None], [0], [9]), 1)
    nodes = pad_bvh2_depth(root, levels) if levels else root
    return gi.pack_objects([obj]), upload_tlas(gi, nodes, inst), (nodes, inst, p_nodes, p_tris)


def chain_rays(n):
    rng = np.random.default_rng(n)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[:, 2] = -1.0
    return F.make_rays(org, np.tile(np.float32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 1000.0)


def test_stack_at_the_limit_and_beyond(gi, oracle):
    import torch
    from rodent_amd import abi
    rays = chain_rays(70)
    _, _, model = chain_scene(gi, 40, 0)
    own = int(M.peak(oracle, *model, rays[:4]).max())
    assert own >= 40
    levels = 62 - own                                        # P + 2 == 64
    objects, tlas, model = chain_scene(gi, 40, levels)
    assert (M.peak(oracle, *model, rays[:4]) == 62).all()
    m_hits, m_ids = M.trace(oracle, *model, rays)
    assert (m_ids == 9).all() and (m_hits["tri_id"] == 0).all()
    stream = torch.cuda.Stream()
    rays_dev = abi.to_device(rays)
    hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
    ids_dev = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gi.trace_async(objects, tlas, rays_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    # an object deeper than the stack: the flag, and nothing else
    deep_objects, deep_tlas, _ = chain_scene(gi, 80, 0)
    gi.trace_async(deep_objects, deep_tlas, rays_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 1
    # the next launch on the stream is clean
    hits_dev.zero_(); ids_dev.zero_()
    torch.cuda.synchronize()
    gi.trace_async(objects, tlas, rays_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    abi.check_errors(0)            # the default stream's context is the one used last again: the library's debug read-outs look at that one


# ---- moved transforms -----------------------------------------------------------------------------------------------------------
def moved_case(cornell):
    transforms, obj, ids = parity_layout()
    moved = transforms.copy().reshape(9, 3, 4)
    moved[:, :, 3] += np.float32([0.6, -0.3, 0.5])
    moved[4, :, :3] = moved[4, :, :3] @ np.float32([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    rays = scene_rays(cornell, 1024, 12)
    return transforms, moved.reshape(9, 12), obj, ids, np.concatenate([rays["camera"][::4], rays["segments"]])


def test_moved_transforms_rebuilt_in_place(gi, oracle, parity, cornell):
    import torch
    from rodent_amd import abi
    objects, _, _, _, (p_nodes, p_tris, table) = parity
    transforms, moved, obj, ids, rays = moved_case(cornell)
    stream = torch.cuda.Stream()
    tlas = gi.build_tlas(objects, transforms, obj, ids, 2, stream=stream)
    rays_dev = abi.to_device(rays)
    out = [(torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda"),
            torch.zeros(len(rays), dtype=torch.int32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    results = []
    for k, t in enumerate((transforms, moved)):
        if k:
            ptrs = (tlas.nodes.data_ptr(), tlas.instances.data_ptr())
            assert gi.build_tlas(objects, t, obj, ids, 2, stream=stream, out=tlas) is tlas
            assert ptrs == (tlas.nodes.data_ptr(), tlas.instances.data_ptr())
        model = M.build_tlas(p_nodes, table, M.descriptors(t, obj, ids), 2)
        same_tlas(gi, tlas, model)
        gi.trace_async(objects, tlas, rays_dev, *out[k], len(rays), False, stream)
        abi.check_errors(0, stream)
        hits, got_ids = abi.from_device(out[k][0], F.HIT1), out[k][1].cpu().numpy()
        m_hits, m_ids = M.trace(oracle, model[0], model[1], p_nodes, p_tris, rays)
        assert hits.tobytes() == m_hits.tobytes() and np.array_equal(got_ids, m_ids)
        results.append(hits)
    changed = int((results[0].view("<u4").reshape(-1, 4) != results[1].view("<u4").reshape(-1, 4)).any(1).sum())
    print(f"{changed} of {len(rays)} rays changed their record")
    assert changed == MOVED_RAYS
    abi.check_errors(0)            # as in the stack test: leave the default stream's context as the one used last


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_on_the_host(gi):
    import torch
    from rodent_amd import abi
    l = abi.lib()
    assert l.rodent_hip_tlas_scratch_bytes(0) == -1 and l.rodent_hip_tlas_scratch_bytes((1 << 22) + 1) == -1
    assert l.rodent_hip_tlas_scratch_bytes(1 << 22) > 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    call = lambda n, max_leaf=1, objects=1: l.rodent_hip_build_tlas(0, p, p, objects, p, n, max_leaf, p, p, p, p, None)
    assert call(0) == gi.ERR_NUM_INSTANCES and call((1 << 22) + 1) == gi.ERR_NUM_INSTANCES and call(-1) == gi.ERR_NUM_INSTANCES
    assert call(1, 0) == -2 and call(1, 9) == -2
    assert call(1, 1, 0) == gi.ERR_NUM_OBJECTS
    for hole in range(7):                                                   # every pointer in turn
        args = [p] * 7
        args[hole] = None
        nodes, objects, descs, tlas_nodes, instances, scratch, info = args
        assert l.rodent_hip_build_tlas(0, nodes, objects, 1, descs, 1, 1, tlas_nodes, instances, scratch, info, None) == -4
    assert l.rodent_hip_build_tlas(99, p, p, 1, p, 1, 1, p, p, p, p, None) == -5
    assert l.rodent_hip_build_tlas_sync(0, p, p, 1, p, 0, 1, p, p, None) == gi.ERR_NUM_INSTANCES
    assert l.rodent_hip_build_tlas_sync(0, p, p, 1, p, 1, 9, p, p, None) == -2
    torch.cuda.synchronize()
    assert not buf.any()                                                    # nothing was enqueued


def test_device_flags_raise_build_errors(gi, two_objects):
    from rodent_amd import gpubuild
    objects, (p_nodes, _, table) = two_objects
    transforms, obj = M.seeded_transforms(100, 5, 40.0, 2)
    for bad_obj in (2, -1):
        o = obj.copy(); o[37] = bad_obj
        with pytest.raises(gpubuild.BuildError, match="object index"):
            gi.build_tlas(objects, transforms, o)
    singular = transforms.copy(); singular[50, 8:11] = singular[50, 0:3]
    nan = transforms.copy(); nan[99, 6] = np.nan
    for t in (singular, nan):
        assert M.build_tlas(p_nodes, table, M.descriptors(t, obj), 1)[2][2] == M.BAD_TRANSFORM
        with pytest.raises(gpubuild.BuildError, match="transform"):
            gi.build_tlas(objects, t, obj)
    for kw in ({"max_leaf": 0}, {"max_leaf": 9}):
        with pytest.raises(gpubuild.BuildError):
            gi.build_tlas(objects, transforms, obj, **kw)
    with pytest.raises(gpubuild.BuildError):
        gi.build_tlas(objects, transforms[:0], obj[:0])
    # the flags are per call
    assert gi.build_tlas(objects, transforms, obj).info[2] == 0
