"""Deforming objects under moving instances on the GPU (the section of that name of include/rodent_instances.h; rodent_amd/instances.py)
against tests/motion_objects_model.py, byte for byte.

* build: the motion records and info words of build_motion_objects equal the model's over build_objects' topologies (max_leaf 1 / 2 / 8)
  and over pack_objects of per-object build_bvh2 with two treelet passes; again in place with other keys; per object they are
  motion.build_motion_bvh2's of that object alone; a bad index and a non-finite coordinate at either key inside one object raise the
  flag, make the synchronous form return RODENT_BUILD_ERR_INPUT and leave the other objects complete;
* TLAS: nodes, instance records and info words equal the model's at max_leaf 1 / 2 / 8; a bad object index and a singular endpoint
  raise their flags; build_motion_tlas over an ObjectSet gives the bytes of motion_instance_model as before;
* trace: hit records and instance ids equal the model's for all four ray sets of tests/motion_objects_fixtures.py with its 23 times
  cycled over the rays (refused beside traced ones in every wave), closest and any hit, both entry forms, without the instance-id array,
  cut to 1 / 63 / 64 / 65 / all rays into buffers filled with 0xA5; one identity instance of one object gives motion.trace_motion's hits;
* stack: P + 2 == 64 at the rays' own time is traced without a flag, the same scene at a time at which the object is deeper raises the
  overflow word, the next launch is clean.
"""
import ctypes as C

import numpy as np
import pytest

import instance_model as M
import lbvh_model as L
import motion_bvh_fixtures as BX
import motion_bvh_model as B
import motion_instance_model as MI
import motion_objects_fixtures as X
import motion_objects_model as MO
from conftest import chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

pytestmark = pytest.mark.gpu
F32 = np.float32
IDENTITY = F32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
ERR_INPUT = -7


@pytest.fixture(scope="module")
def gi(native_build):
    import torch
    from rodent_amd import instances
    assert torch.cuda.is_available(), "these tests need a GPU"
    return instances


@pytest.fixture(scope="module")
def block(cornell):
    return cornell.blocks[2]


@pytest.fixture(scope="module")
def scene(block):
    return X.Scene(block)


@pytest.fixture(scope="module")
def placed(gi, scene):
    """The fixture on the device: its topologies packed, the motion records built over them, its motion TLAS -- each checked against
    the model's bytes."""
    objects = gi.pack_objects(scene.pairs)
    mo = gi.build_motion_objects(objects, scene.v0, scene.v1, scene.ix, scene.ranges)
    same_records(gi, mo, scene.mn, scene.mt, scene.build_info)
    tlas = gi.build_motion_tlas(mo, scene.t0, scene.t1, scene.obj, scene.ids, 1)
    same_tlas(gi, tlas, (scene.tlas, scene.inst, scene.info))
    return mo, tlas


@pytest.fixture(scope="module")
def expected(oracle, scene, cornell):
    """{(name, any_hit): (rays, times, model hits, model ids)}, computed once."""
    return {(name, any_hit): (rays, X.times_for(len(rays)), *MO.trace(oracle, *scene.model(), rays, X.times_for(len(rays)), any_hit))
            for name, rays in X.ray_sets(cornell).items() for any_hit in (False, True)}


def same_records(gi, mo, mn, mt, info):
    nodes, tris = gi.download_motion_objects(mo)
    assert np.array_equal(mo.info, info), (mo.info, info)
    assert nodes.tobytes() == mn.tobytes() and tris.tobytes() == mt.tobytes()


def same_tlas(gi, tlas, model):
    nodes, inst = gi.download_motion(tlas)
    m_nodes, m_inst, m_info = model
    assert np.array_equal(tlas.info, m_info), (tlas.info, m_info)
    assert nodes.tobytes() == m_nodes.tobytes() and inst.tobytes() == m_inst.tobytes()


# ---- 1. build -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [1, 2, 8])
def test_build_over_build_objects_equals_the_model(gi, block, max_leaf):
    sc = X.Scene(block, topology_leaf=max_leaf)
    objects = gi.build_objects(sc.v0, sc.ix, sc.ranges, max_leaf)
    assert np.array_equal(objects.table, sc.table)
    mo = gi.build_motion_objects(objects, sc.v0, sc.v1, sc.ix, sc.ranges)
    same_records(gi, mo, sc.mn, sc.mt, sc.build_info)
    # again, in place, with the keys exchanged: the refit of a motion set
    ptrs = (mo.nodes.data_ptr(), mo.tris.data_ptr(), mo.scratch.data_ptr())
    again = gi.build_motion_objects(objects, sc.v1, sc.v0, sc.ix, gi.plan_refit(objects, np.arange(5), sc.ranges), out=mo)
    assert again is mo and ptrs == (mo.nodes.data_ptr(), mo.tris.data_ptr(), mo.scratch.data_ptr())
    same_records(gi, mo, *MO.build(sc.nodes, sc.tris, sc.table, sc.v1, sc.v0, sc.ix, sc.ranges))


def test_build_over_treelet_topologies_and_per_object_bytes(gi, scene):
    from rodent_amd import gpubuild, motion
    bvhs = [gpubuild.build_bvh2(scene.v0, scene.ix[first: first + count], 2, treelet_passes=2) for first, count in scene.ranges]
    pairs = [gpubuild.download(b) for b in bvhs]
    nodes, tris, table = M.pack(pairs)
    assert nodes.tobytes() != scene.nodes.tobytes()                                     # another topology than the LBVH's
    objects = gi.pack_objects(bvhs)
    mo = gi.build_motion_objects(objects, scene.v0, scene.v1, scene.ix, scene.ranges)
    mn, mt, info = MO.build(nodes, tris, table, scene.v0, scene.v1, scene.ix, scene.ranges)
    assert info.tolist() == [len(nodes), len(nodes) + len(tris), 0, len(nodes)]
    same_records(gi, mo, mn, mt, info)
    got_n, got_t = gi.download_motion_objects(mo)
    for bvh, ob, (first, count) in zip(bvhs, table, scene.ranges):                      # per object: the single-mesh build's bytes
        alone = motion.download(motion.build_motion_bvh2(bvh, scene.v0, scene.v1, scene.ix[first: first + count]))
        assert got_n[ob["node_offset"]:][: ob["num_nodes"]].tobytes() == alone[0].tobytes()
        assert got_t[ob["tri_offset"]:][: ob["num_tris"]].tobytes() == alone[1].tobytes()
    # pack_motion_objects of the single-mesh builds is the same set
    packed = gi.pack_motion_objects([motion.build_motion_bvh2(b, scene.v0, scene.v1, scene.ix[f: f + c])
                                     for b, (f, c) in zip(bvhs, scene.ranges)])
    assert np.array_equal(packed.table, table)
    assert [a.tobytes() for a in gi.download_motion_objects(packed)] == [mn.tobytes(), mt.tobytes()]


def test_a_fault_inside_one_object_leaves_the_others_complete(gi, scene):
    from rodent_amd import abi, gpubuild
    objects = gi.pack_objects(scene.pairs)
    first, count = scene.ranges[X.SOUP]
    bad_ix = scene.ix.copy(); bad_ix[first + 7, 1] = len(scene.v0)
    row = scene.ix[first + 11, 0]
    nan0, inf1 = scene.v0.copy(), scene.v1.copy()
    nan0[row, 1], inf1[row, 2] = np.nan, np.inf
    plan = gi.plan_refit(objects, np.arange(5), scene.ranges)
    total = len(scene.nodes)
    for v0, v1, ix, flag in ((scene.v0, scene.v1, bad_ix, L.BAD_INDEX), (nan0, scene.v1, scene.ix, L.NON_FINITE),
                             (scene.v0, inf1, scene.ix, L.NON_FINITE)):
        mo = gi.build_motion_objects(objects, v0, v1, ix, plan, check=False)
        model = MO.build(scene.nodes, scene.tris, scene.table, v0, v1, ix, scene.ranges)[2]
        assert model[2] == flag and mo.info.tolist() == model.tolist(), (mo.info, model)
        got_n, got_t = gi.download_motion_objects(mo)
        for k, ob in enumerate(scene.table):
            if k != X.SOUP:
                ns, ts = slice(ob["node_offset"], ob["node_offset"] + ob["num_nodes"]), slice(ob["tri_offset"], ob["tri_offset"] + ob["num_tris"])
                assert got_n[ns].tobytes() == scene.mn[ns].tobytes() and got_t[ts].tobytes() == scene.mt[ts].tobytes(), (flag, k)
        with pytest.raises(gpubuild.BuildError):
            gi.build_motion_objects(objects, v0, v1, ix, plan)
        # the synchronous entry
        d0, d1, dix = (gpubuild._columns4(a, t, 0) for a, t in ((v0, gi.torch.float32), (v1, gi.torch.float32), (ix, gi.torch.int32)))
        info = (C.c_int32 * 4)()
        gi.torch.cuda.synchronize()
        rc = abi.lib().rodent_hip_build_motion_objects_sync(
            0, d0.data_ptr(), d1.data_ptr(), len(v0), dix.data_ptr(), len(ix), objects.nodes.data_ptr(), total, objects.tris.data_ptr(),
            len(scene.tris), objects.table_dev.data_ptr(), 5, plan.table_dev.data_ptr(), 5, plan.num_nodes, plan.num_recs,
            mo.nodes.data_ptr(), mo.tris.data_ptr(), info)
        assert rc == ERR_INPUT and list(info) == mo.info.tolist()
    info = (C.c_int32 * 4)()
    d0, d1, dix = (gpubuild._columns4(a, t, 0) for a, t in ((scene.v0, gi.torch.float32), (scene.v1, gi.torch.float32),
                                                            (scene.ix, gi.torch.int32)))
    gi.torch.cuda.synchronize()
    rc = abi.lib().rodent_hip_build_motion_objects_sync(
        0, d0.data_ptr(), d1.data_ptr(), len(scene.v0), dix.data_ptr(), len(scene.ix), objects.nodes.data_ptr(), total,
        objects.tris.data_ptr(), len(scene.tris), objects.table_dev.data_ptr(), 5, plan.table_dev.data_ptr(), 5, plan.num_nodes,
        plan.num_recs, mo.nodes.data_ptr(), mo.tris.data_ptr(), info)
    assert rc == 0 and list(info) == scene.build_info.tolist()
    same_records(gi, gi.MotionObjectSet(mo.buffer, mo.nodes, mo.tris, mo.table, mo.table_dev, 0, scene.build_info), scene.mn, scene.mt,
                 scene.build_info)


# ---- 2. TLAS ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [1, 2, 8])
def test_tlas_bytes_equal_the_model(gi, placed, scene, max_leaf):
    mo, _ = placed
    model = MO.build_motion_tlas(scene.mn, scene.table, scene.descs, max_leaf)
    assert model[2][2] == 0
    same_tlas(gi, gi.build_motion_tlas(mo, scene.t0, scene.t1, scene.obj, scene.ids, max_leaf), model)
    seeded0, obj = M.seeded_transforms(64, 11 + max_leaf, 40.0, 5)                    # 64 seeded instances of the five objects
    seeded1, _ = M.seeded_transforms(64, 111 + max_leaf, 40.0, 5)
    ids = (np.arange(64) * 3 + 1).astype(np.int64)
    model = MO.build_motion_tlas(scene.mn, scene.table, MI.descriptors(seeded0, seeded1, obj, ids), max_leaf)
    assert model[2][2] == 0
    same_tlas(gi, gi.build_motion_tlas(mo, seeded0, seeded1, obj, ids, max_leaf), model)


def test_tlas_flags_and_the_static_sets_bytes(gi, placed, scene):
    from rodent_amd import gpubuild
    mo, _ = placed
    bad_obj = scene.obj.copy(); bad_obj[4] = 5
    singular = scene.t1.copy(); singular[2, 8:11] = singular[2, 0:3]
    for t1, obj, flag, words in ((scene.t1, bad_obj, M.BAD_OBJECT, "object index"), (singular, scene.obj, M.BAD_TRANSFORM, "transform")):
        assert MO.build_motion_tlas(scene.mn, scene.table, MI.descriptors(scene.t0, t1, obj, scene.ids), 2)[2][2] == flag
        with pytest.raises(gpubuild.BuildError, match=words):
            gi.build_motion_tlas(mo, scene.t0, t1, obj, scene.ids, 2)
    # an ObjectSet goes through the entry it always went through: motion_instance_model's bytes, which differ from the motion set's
    static = gi.pack_objects(scene.pairs)
    model = MI.build_motion_tlas(scene.nodes, scene.table, scene.descs, 2)
    same_tlas(gi, gi.build_motion_tlas(static, scene.t0, scene.t1, scene.obj, scene.ids, 2), model)
    assert model[0].tobytes() != MO.build_motion_tlas(scene.mn, scene.table, scene.descs, 2)[0].tobytes()


# ---- 3. trace -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name", ["primary", "random", "edge", "segments"])
def test_trace_equals_the_model(gi, placed, expected, name, any_hit):
    import torch
    from rodent_amd import abi
    mo, tlas = placed
    rays, times, m_hits, m_ids = expected[(name, any_hit)]
    on = B.traced(times[:64])
    assert on.any() and (~on).any()                                                     # refused beside traced times in one wave
    assert (m_hits["tri_id"][B.traced(times)] >= 0).mean() >= 0.25
    hits, ids = gi.trace_motion(mo, tlas, rays, times, any_hit)                         # the synchronous entries
    assert hits.tobytes() == m_hits.tobytes() and np.array_equal(ids, m_ids)
    assert not np.isnan(hits["u"]).any() and not np.isnan(hits["v"]).any()
    # the asynchronous entry, cut to 1 / 63 / 64 / 65 / all rays, into buffers filled with 0xA5; with and without the instance-id array
    n = len(rays)
    rays_dev, times_dev = abi.to_device(rays), torch.from_numpy(times).cuda()
    for count in (1, 63, 64, 65, n):
        for with_ids in (True, False):
            hits_dev = torch.full((n * F.HIT1.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            ids_dev = torch.full((n * 4,), 0xA5, dtype=torch.uint8, device="cuda")
            gi.trace_motion_async(mo, tlas, rays_dev, times_dev, hits_dev, ids_dev.view(torch.int32) if with_ids else None, count, any_hit)
            abi.check_errors(0)
            got, got_ids = hits_dev.cpu().numpy(), ids_dev.cpu().numpy()
            assert got[: count * 16].tobytes() == m_hits[:count].tobytes(), (name, any_hit, count)
            assert (got[count * 16:] == 0xA5).all()
            if with_ids:
                assert np.array_equal(got_ids[: count * 4].view(np.int32), m_ids[:count]) and (got_ids[count * 4:] == 0xA5).all()
            else:
                assert (got_ids == 0xA5).all()


def test_one_identity_instance_gives_the_single_mesh_trace(gi, scene):
    from rodent_amd import gpubuild, motion
    first, count = scene.ranges[X.SOUP]
    rows = scene.ix[first: first + count]
    mbvh = motion.build_motion_bvh2(gpubuild.build_bvh2(scene.v0, rows, 2), scene.v0, scene.v1, rows)
    mo = gi.pack_motion_objects([mbvh])
    tlas = gi.build_motion_tlas(mo, IDENTITY[None], IDENTITY[None], [0], [5])
    rays = BX.segments(np.full(3, -0.7), np.full(3, 0.7), 1024, 5)
    times = X.times_for(len(rays))
    for any_hit in (False, True):
        want = motion.trace_motion(mbvh, rays, times, any_hit)
        hits, ids = gi.trace_motion(mo, tlas, rays, times, any_hit)
        assert hits.tobytes() == want.tobytes() and np.array_equal(ids, np.where(want["tri_id"] >= 0, 5, -1))
        assert (want["tri_id"][B.traced(times)] >= 0).mean() > 0.25


# ---- 4. stack -----------------------------------------------------------------------------------------------------------------------------
GATE, DEPTH = 30, 56                # (the object alone stays within the oracle's own 64 entries at either time)


def gated_chain():
    """conftest.chain_bvh2(DEPTH) as a motion object whose chain below level GATE lies beside the rays at key 0 (the box of node GATE's
    inner child is moved to x in [1000, 1010]) and where chain_bvh2 put it at key 1: a ray's peak is about GATE at time 0 and DEPTH at
    time 1."""
    nodes, tris = chain_bvh2(DEPTH)
    beside = nodes.copy()
    b = beside["bounds"][GATE].copy(); b[0:2] = [1000, 1010]; beside["bounds"][GATE] = b
    mn, mt, info = B.fuse(beside, tris, nodes, tris)
    assert info[2] == 0
    return mn, mt


def chain_scene(gi, levels):
    """The gated chain under one instance that shifts by 1/4 along x between its placements, whose single-leaf motion TLAS is padded by
    `levels` nodes."""
    from rodent_amd import abi
    mn, mt = gated_chain()
    table = M.pack([(np.zeros(len(mn), F.NODE2), np.zeros(len(mt), F.TRI1))])[2]
    moved = IDENTITY.copy(); moved[3] = 0.25
    root, inst, info = MO.build_motion_tlas(mn, table, MI.descriptors(IDENTITY[None], moved[None], [0], [9]), 1)
    assert info[2] == 0
    nodes = pad_bvh2_depth(root, levels) if levels else root
    tlas = gi.MotionTlas(abi.to_device(nodes), abi.to_device(inst), len(inst), np.int32([len(nodes), 1, 0, 0]), None, 0)
    return gi.pack_motion_objects([(mn, mt)]), tlas, (nodes, inst, mn, mt)


def chain_rays(n):
    rng = np.random.default_rng(n)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[:, 2] = -1.0
    return F.make_rays(org, np.tile(F32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 1000.0)


def test_stack_at_the_limit_at_the_rays_time_and_beyond_at_another(gi, oracle):
    import torch
    from rodent_amd import abi
    rays = chain_rays(70)
    early = F32([0.0, 0.25, 0.5, -0.0])[np.arange(70) % 4]                               # the chain below GATE lies beside the rays
    late = np.ones(70, F32)
    _, _, model = chain_scene(gi, 0)
    own = int(MO.peak(oracle, *model, rays[:4], early[:4]).max())
    assert GATE <= own < 62 and int(MO.peak(oracle, *model, rays[:1], late[:1])[0]) >= DEPTH
    levels = 62 - own                                                                    # P + 2 == 64 at the early times
    mo, tlas, model = chain_scene(gi, levels)
    assert (MO.peak(oracle, *model, rays[:4], early[:4]) == 62).all()
    assert (MO.peak(oracle, *model, rays[:4], late[:4]) > 62).all()                      # ... and deeper at time 1
    m_hits, m_ids = MO.trace(oracle, *model, rays, early)
    assert (m_ids == 9).all() and (m_hits["tri_id"] == 0).all()
    stream = torch.cuda.Stream()
    rays_dev, early_dev, late_dev = abi.to_device(rays), torch.from_numpy(early).cuda(), torch.from_numpy(late).cuda()
    hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
    ids_dev = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gi.trace_motion_async(mo, tlas, rays_dev, early_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    # the same scene at the time at which the object is deeper: the overflow word, and nothing else
    gi.trace_motion_async(mo, tlas, rays_dev, late_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 1
    # the next launch on the stream is clean
    hits_dev.zero_(); ids_dev.zero_()
    torch.cuda.synchronize()
    gi.trace_motion_async(mo, tlas, rays_dev, early_dev, hits_dev, ids_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes() and np.array_equal(ids_dev.cpu().numpy(), m_ids)
    abi.check_errors(0)            # the default stream's context is the one used last again
