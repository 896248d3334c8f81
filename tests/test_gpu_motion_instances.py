"""Moving instances on the GPU (the section "moving instances" of include/rodent_instances.h; rodent_amd/instances.py) against
tests/motion_instance_model.py.

* the motion TLAS's nodes, RodentMotionInstance records and info words equal the model's byte for byte (1, 2, 9, 64 and 64 coincident
  instances, max_leaf 1 / 2 / 8), also rebuilt in place on a second stream;
* hit records and instance ids equal the model's exactly: the fixture of tests/motion_instance_fixtures.py, both ray sets, a 16-value
  palette of times (NaN, a denormal and times outside [0, 1] among them), closest and any hit, cut to 1, 4096 + 37 and 64 k rays;
* all times 0: the records of the static trace over M0;
* the half-turn instance at t = 0.5 is skipped: no flag, no NaN, the rays hit what lies behind it;
* the device flags for a bad M0 alone, a bad M1 alone and a bad object, with guard bytes around everything the build writes;
* the stack: P + 2 == 64 is traced, a deeper object raises the overflow word on the asynchronous entry, the next launch is clean.
"""
import ctypes as C

import numpy as np
import pytest

import instance_edge_fixtures as E
import instance_model as M
import motion_instance_fixtures as X
import motion_instance_model as MM
from conftest import chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

pytestmark = pytest.mark.gpu
F32 = np.float32
IDENTITY = F32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


@pytest.fixture(scope="module")
def gi(native_build):
    import torch
    from rodent_amd import instances
    assert torch.cuda.is_available(), "these tests need a GPU"
    return instances


@pytest.fixture(scope="module")
def scene(cornell):
    return X.Scene(cornell.blocks[2])


@pytest.fixture(scope="module")
def placed(gi, scene):
    """The fixture's objects and its motion TLAS on the device, the latter checked against the model's."""
    objects = gi.pack_objects(scene.pairs)
    tlas = gi.build_motion_tlas(objects, scene.t0, scene.t1, scene.obj, scene.ids, 1)
    same_tlas(gi, tlas, (scene.tlas, scene.inst, scene.info))
    return objects, tlas


@pytest.fixture(scope="module")
def expected(oracle, scene, cornell):
    """{(name, any_hit): (rays, times, model hits, model ids)}, computed once."""
    return {(name, any_hit): (rays, times, *MM.trace(oracle, *scene.model(), rays, times, any_hit))
            for name, (rays, times) in X.ray_sets(cornell).items() for any_hit in (False, True)}


def same_tlas(gi, tlas, model):
    nodes, inst = gi.download_motion(tlas)
    m_nodes, m_inst, m_info = model
    assert np.array_equal(tlas.info, m_info), (tlas.info, m_info)
    assert nodes.tobytes() == m_nodes.tobytes() and inst.tobytes() == m_inst.tobytes()


# ---- 1. TLAS bytes ------------------------------------------------------------------------------------------------------------------------
def seeded_pair(n, seed):
    """n seeded instances of two objects and their second placements (instance_model.seeded_transforms twice: instance 1 coincides
    with instance 0 at both ends)."""
    t0, obj = M.seeded_transforms(n, seed, 40.0, 2)
    t1, _ = M.seeded_transforms(n, seed + 1000, 40.0, 2)
    return t0, t1, obj, (np.arange(n) * 7 + 5).astype(np.int64)


def coincident(n=64):
    moved = E.COINCIDENT.copy(); moved[3::4] += F32([0.5, -0.25, 0.125])
    return np.tile(E.COINCIDENT, (n, 1)), np.tile(moved, (n, 1)), np.zeros(n, np.int32), np.arange(n).astype(np.int64)


@pytest.fixture(scope="module")
def two_objects(gi, cornell):
    pairs = [cornell.blocks[2], M.flat_object()]
    return gi.pack_objects(pairs), M.pack(pairs)


@pytest.mark.parametrize("max_leaf", [1, 2, 8])
def test_tlas_bytes_equal_the_model(gi, two_objects, max_leaf):
    objects, (p_nodes, _, table) = two_objects
    for case in [seeded_pair(n, 100 * max_leaf + n) for n in (1, 2, 9, 64)] + [coincident()]:
        t0, t1, obj, ids = case
        model = MM.build_motion_tlas(p_nodes, table, MM.descriptors(t0, t1, obj, ids), max_leaf)
        assert model[2][2] == 0
        same_tlas(gi, gi.build_motion_tlas(objects, t0, t1, obj, ids, max_leaf), model)


def test_tlas_rebuilt_in_place_on_a_second_stream(gi, two_objects):
    import torch
    objects, (p_nodes, _, table) = two_objects
    stream = torch.cuda.Stream()
    big = gi.build_motion_tlas(objects, *seeded_pair(64, 7), max_leaf=2)
    ptrs = (big.nodes.data_ptr(), big.instances.data_ptr(), big.scratch.data_ptr())
    t0, t1, obj, ids = seeded_pair(9, 8)
    for a, b in ((t0, t1), (t1, t0)):                                   # two frames: device tensors in, no host copy of them
        out = gi.build_motion_tlas(objects, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), obj, ids, 2, stream=stream, out=big)
        assert out is big and ptrs == (big.nodes.data_ptr(), big.instances.data_ptr(), big.scratch.data_ptr())
        same_tlas(gi, big, MM.build_motion_tlas(p_nodes, table, MM.descriptors(a, b, obj, ids), 2))


# ---- 2. trace -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name", ["primary", "random"])
def test_trace_equals_the_model(gi, placed, expected, name, any_hit):
    import torch
    from rodent_amd import abi
    objects, tlas = placed
    rays, times, m_hits, m_ids = expected[(name, any_hit)]
    assert len(set(bits(times))) == 16
    for count in (len(rays), 1, 64 * 5):
        hits, ids = gi.trace_motion(objects, tlas, rays[:count], times[:count], any_hit)
        assert hits.tobytes() == m_hits[:count].tobytes(), (name, any_hit, count)
        assert np.array_equal(ids, m_ids[:count]), (name, any_hit, count)
    assert not np.isnan(hits["u"]).any() and not np.isnan(hits["v"]).any()
    # the asynchronous entry without the instance-id array: the same hit records
    rays_dev, times_dev = abi.to_device(rays), torch.from_numpy(times).cuda()
    hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
    gi.trace_motion_async(objects, tlas, rays_dev, times_dev, hits_dev, None, len(rays), any_hit)
    abi.check_errors(0)
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes()


def bits(a):
    return np.ascontiguousarray(a, F32).view("<u4")


@pytest.mark.parametrize("any_hit", [False, True])
def test_trace_of_both_sets_cut_past_a_chunk(gi, placed, expected, any_hit):
    """4096 + 37 rays: the primary set and the start of the segments, the last chunk partly filled."""
    objects, tlas = placed
    parts = [expected[(name, any_hit)] for name in ("primary", "random")]
    n = 4096 + 37
    rays, times, m_hits, m_ids = (np.concatenate([p[k] for p in parts])[:n] for k in range(4))
    hits, ids = gi.trace_motion(objects, tlas, rays, times, any_hit)
    assert hits.tobytes() == m_hits.tobytes() and np.array_equal(ids, m_ids)


# ---- 3. all times 0 -----------------------------------------------------------------------------------------------------------------------
def test_all_times_zero_equals_the_static_trace_over_m0(gi, placed, scene, cornell):
    """No two instances of the fixture coincide, so the static TLAS over M0 (another tree) gives the same closest hits; the CPU test
    asserts that the models say so."""
    objects, tlas = placed
    static = gi.build_tlas(objects, scene.t0, scene.obj, scene.ids, 1)
    for name, (rays, _) in X.ray_sets(cornell).items():
        a = gi.trace_motion(objects, tlas, rays, np.zeros(len(rays), F32))
        b = gi.trace(objects, static, rays)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), name
        assert (a[0]["tri_id"] >= 0).mean() > 0.3


# ---- 4. the half turn ---------------------------------------------------------------------------------------------------------------------
def test_half_turn_instance_is_skipped_at_half(gi, oracle, placed, scene):
    import torch
    from rodent_amd import abi
    objects, tlas = placed
    rays = X.half_turn_rays(scene)
    own = int(scene.ids[X.HALF_TURN])
    for t in (0.0, 0.5):
        times = np.full(len(rays), t, F32)
        m_hits, m_ids = MM.trace(oracle, *scene.model(), rays, times)
        rays_dev, times_dev = abi.to_device(rays), torch.from_numpy(times).cuda()
        hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        ids_dev = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
        gi.trace_motion_async(objects, tlas, rays_dev, times_dev, hits_dev, ids_dev, len(rays))
        assert abi.lib().rodent_hip_check_errors(0, None) == 0                              # no flag
        hits, ids = abi.from_device(hits_dev, F.HIT1), ids_dev.cpu().numpy()
        assert hits.tobytes() == m_hits.tobytes() and np.array_equal(ids, m_ids)
        assert not np.isnan(hits.view("<f4").reshape(-1, 4)[:, 1:]).any()
        if t == 0.0:
            assert (ids == own).all()
            front = hits["t"].copy()
        else:
            assert (ids != own).all() and (ids >= 0).mean() > 0.9 and (hits["t"][ids >= 0] > front[ids >= 0]).all()


# ---- 5. flags, and guard bytes around everything the build writes -----------------------------------------------------------------------
GUARD = 256


def guarded(nbytes):
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def test_device_flags_and_guard_bytes(gi, two_objects):
    import torch
    from rodent_amd import abi, gpubuild
    objects, (p_nodes, _, table) = two_objects
    n = 100
    t0, t1, obj, ids = seeded_pair(n, 5)
    singular = t0.copy(); singular[50, 8:11] = singular[50, 0:3]
    nan = t1.copy(); nan[99, 6] = np.nan
    bad_obj = obj.copy(); bad_obj[37] = 2
    negative = obj.copy(); negative[0] = -1
    cases = [(t0, t1, obj, 0), (singular, t1, obj, M.BAD_TRANSFORM), (t0, singular, obj, M.BAD_TRANSFORM), (nan, t1, obj, M.BAD_TRANSFORM),
             (t0, nan, obj, M.BAD_TRANSFORM), (t0, t1, bad_obj, M.BAD_OBJECT), (t0, t1, negative, M.BAD_OBJECT),
             (singular, nan, bad_obj, M.BAD_OBJECT | M.BAD_TRANSFORM)]
    l = abi.lib()
    need = l.rodent_hip_motion_tlas_scratch_bytes(n)
    for a, b, o, flag in cases:
        descs = MM.descriptors(a, b, o, ids)
        assert MM.build_motion_tlas(p_nodes, table, descs, 2)[2][2] == flag
        bufs = [guarded((n - 1) * F.NODE2.itemsize), guarded(n * F.MOTION_INSTANCE.itemsize), guarded(need), guarded(16)]
        (_, nodes), (_, inst), (_, scratch), (info_buf, info) = bufs
        descs_buf, descs_dev = guarded(descs.nbytes)
        descs_buf[GUARD:GUARD + descs.nbytes] = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        rc = l.rodent_hip_build_motion_tlas(0, objects.nodes.data_ptr(), objects.table_dev.data_ptr(), objects.num_objects, descs_dev, n, 2,
                                            nodes, inst, scratch, info, None)
        torch.cuda.synchronize()
        assert rc == 0
        words = info_buf[GUARD:GUARD + 16].cpu().numpy().view(np.int32)
        assert words[2] == flag and words[3] == 0, (words, flag)
        assert all(guards_intact(buf) for buf, _ in bufs) and guards_intact(descs_buf)
        assert descs_buf[GUARD:GUARD + descs.nbytes].cpu().numpy().tobytes() == descs.tobytes()
        # the Python entry: a BuildError naming the flag, nothing raised for the sound call
        if flag == 0:
            assert gi.build_motion_tlas(objects, a, b, o, ids, 2).info[2] == 0
        else:
            with pytest.raises(gpubuild.BuildError, match="object index" if flag & M.BAD_OBJECT else "transform"):
                gi.build_motion_tlas(objects, a, b, o, ids, 2)
    for kw in ({"max_leaf": 0}, {"max_leaf": 9}):
        with pytest.raises(gpubuild.BuildError):
            gi.build_motion_tlas(objects, t0, t1, obj, **kw)
    with pytest.raises(ValueError):
        gi.build_motion_tlas(objects, t0, t1[:50], obj)


# ---- 6. stack (the construction of tests/test_gpu_instances.py, restated over motion records) ------------------------------------------
def upload_tlas(gi, nodes, inst):
    from rodent_amd import abi
    return gi.MotionTlas(abi.to_device(nodes), abi.to_device(inst), len(inst), np.int32([len(nodes), 1, 0, 0]), None, 0)


def chain_scene(gi, depth, levels):
    """conftest.chain_bvh2(depth) as the one object, under one instance that shifts by 1/4 along x between its two placements, whose
    single-leaf motion TLAS is padded by `levels` nodes."""
    obj = chain_bvh2(depth)
    p_nodes, p_tris, table = M.pack([obj])
    moved = IDENTITY.copy(); moved[3] = 0.25
    root, inst, _ = MM.build_motion_tlas(p_nodes, table, MM.descriptors(IDENTITY[None], moved[None], [0], [9]), 1)
    nodes = pad_bvh2_depth(root, levels) if levels else root
    return gi.pack_objects([obj]), upload_tlas(gi, nodes, inst), (nodes, inst, p_nodes, p_tris)


def chain_rays(n):
    rng = np.random.default_rng(n)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[:, 2] = -1.0
    return F.make_rays(org, np.tile(F32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 1000.0)


def test_stack_at_the_limit_and_beyond(gi, oracle):
    import torch
    from rodent_amd import abi
    rays = chain_rays(70)
    times = F32([0.0, 1.0, 0.5, 0.25])[np.arange(70) % 4]
    _, _, model = chain_scene(gi, 40, 0)
    own = int(MM.peak(oracle, *model, rays[:4], times[:4]).max())
    assert own >= 40
    levels = 62 - own                                        # P + 2 == 64
    objects, tlas, model = chain_scene(gi, 40, levels)
    assert (MM.peak(oracle, *model, rays[:4], times[:4]) == 62).all()
    m_hits, m_ids = MM.trace(oracle, *model, rays, times)
    assert (m_ids == 9).all() and (m_hits["tri_id"] == 0).all()
    stream = torch.cuda.Stream()
    rays_dev, times_dev = abi.to_device(rays), torch.from_numpy(times).cuda()
    hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
    ids_dev = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gi.trace_motion_async(objects, tlas, rays_dev, times_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    # an object deeper than the stack: the flag, and nothing else
    deep_objects, deep_tlas, _ = chain_scene(gi, 80, 0)
    gi.trace_motion_async(deep_objects, deep_tlas, rays_dev, times_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 1
    # the next launch on the stream is clean
    hits_dev.zero_(); ids_dev.zero_()
    torch.cuda.synchronize()
    gi.trace_motion_async(objects, tlas, rays_dev, times_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    abi.check_errors(0)            # the default stream's context is the one used last again
