"""Deforming meshes under motion on the GPU (include/rodent_motion.h; rodent_amd/motion.py) against tests/motion_bvh_model.py.

1. build: the motion records and info words of build_motion_bvh2 over build_bvh2 trees (max_leaf 1 / 2 / 4 / 8 with two treelet passes,
   and a PLOC tree) equal the model's fuse of refit_model.refit at both keys byte for byte; a second call with out= and other keys
   equals a fresh build;
2. fuse: two refits of one topology fuse to the build's bytes; two trees of different topology raise RODENT_BUILD_BAD_TOPOLOGY;
3. build flags: a bad index (the index table serves both keys, so both refits raise it) and a non-finite coordinate at key 1 only, at
   key 0 only and beside the bad index come through the build, its Python entry and its synchronous C form;
4. trace: hit records equal the model's byte for byte -- both shapes, every ray class, 16 times cycled over the rays (7 of them refused),
   closest and any hit, the synchronous and the asynchronous entry, launches of 1, 63, 64, 65 and all rays;
5. static anchor: all times 0 (then 1) give the t of hip_traverse_bvh2_tri1_async over the static tree refitted to that key;
6. stack: a peak of 63 is traced and equals the model, a peak of 64 raises the overflow word, the next launch is clean;
7. time rule: refused times store exact miss records beside traced neighbours in one wave.
"""
import ctypes as C

import numpy as np
import pytest

import motion_bvh_fixtures as X
import motion_bvh_model as MB
import refit_model as R
from conftest import GOLDEN, chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def gpu(native_build):
    import torch
    from rodent_amd import abi, gpubuild, motion
    assert torch.cuda.is_available(), "these tests need a GPU"

    class Gpu:
        pass
    Gpu.abi, Gpu.build, Gpu.motion, Gpu.torch = abi, gpubuild, motion, torch
    return Gpu


@pytest.fixture(scope="module")
def shapes(native_build, cornell, tmp_path_factory):
    from rodent_amd import scene as S
    return X.shapes(S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene"), cornell)


@pytest.fixture(scope="module")
def placed(gpu, oracle, shapes):
    """{shape name: (shape, topology DeviceBvh, MotionBvh, model nodes, model tris)} over build_bvh2(max_leaf 2, two treelet passes) of
    key 0; the device records are held to the model here, and the model to the fixtures' conditions."""
    out = {}
    for sh in shapes:
        bvh = gpu.build.build_bvh2(sh.v0, sh.ix, max_leaf=2, treelet_passes=2)
        mbvh = gpu.motion.build_motion_bvh2(bvh, sh.v0, sh.v1, sh.ix)
        mn, mt = sh.records(*gpu.build.download(bvh))
        same_records(gpu, mbvh, mn, mt)
        X.check_conditions(oracle, sh, mn, mt)
        out[sh.name] = (sh, bvh, mbvh, mn, mt)
    return out


@pytest.fixture(scope="module")
def expected(oracle, placed):
    """{(shape, class, any_hit): (rays, times, model hits)}, computed once."""
    return {(name, cls, any_hit): (rays, X.times_for(len(rays)), MB.trace(oracle, mn, mt, rays, X.times_for(len(rays)), any_hit))
            for name, (sh, _, _, mn, mt) in placed.items() for cls, rays in sh.rays.items() for any_hit in (False, True)}


def same_records(gpu, mbvh, mn, mt):
    nodes, tris = gpu.motion.download(mbvh)
    assert nodes.tobytes() == mn.tobytes()
    assert tris.tobytes() == mt.tobytes()


# ---- 1. build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(max_leaf=1, treelet_passes=2), dict(max_leaf=2, treelet_passes=2),
                                     dict(max_leaf=4, treelet_passes=2), dict(max_leaf=8, treelet_passes=2),
                                     dict(max_leaf=2, ploc_radius=16)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_build_equals_the_model(gpu, shapes, options):
    for sh in shapes:
        bvh = gpu.build.build_bvh2(sh.v0, sh.ix, **options)
        nodes, tris = gpu.build.download(bvh)
        mbvh = gpu.motion.build_motion_bvh2(bvh, sh.v0, sh.v1, sh.ix)
        mn, mt, info = MB.build(nodes, tris, sh.v0, sh.v1, sh.ix)
        assert mbvh.info.tolist() == info.tolist() == [len(nodes), len(nodes) + len(tris), 0, len(nodes)], (sh.name, mbvh.info)
        same_records(gpu, mbvh, mn, mt)
        # the topology was only read
        again = gpu.build.download(bvh)
        assert again[0].tobytes() == nodes.tobytes() and again[1].tobytes() == tris.tobytes()
        # the refit of a motion hierarchy: the same call with other keys, in place, device tensors in
        ptrs = (mbvh.nodes.data_ptr(), mbvh.tris.data_ptr(), mbvh.scratch.data_ptr())
        moved = X.displace(sh.v0, 77, 0.05)
        out = gpu.motion.build_motion_bvh2(bvh, gpu.torch.from_numpy(sh.v1).cuda(), gpu.torch.from_numpy(moved).cuda(), sh.ix, out=mbvh)
        assert out is mbvh and ptrs == (mbvh.nodes.data_ptr(), mbvh.tris.data_ptr(), mbvh.scratch.data_ptr())
        mn2, mt2, info2 = MB.build(nodes, tris, sh.v1, moved, sh.ix)
        assert mbvh.info.tolist() == info2.tolist()
        same_records(gpu, mbvh, mn2, mt2)
        same_records(gpu, gpu.motion.build_motion_bvh2(bvh, sh.v1, moved, sh.ix), mn2, mt2)


# ---- 2. fuse ----------------------------------------------------------------------------------------------------------------------------
def test_fuse_of_one_topology_and_of_two(gpu, shapes):
    sh = shapes[1]
    keys = [gpu.build.refit_bvh2(gpu.build.build_bvh2(sh.v0, sh.ix, max_leaf=2, treelet_passes=2), v, sh.ix) for v in (sh.v0, sh.v1)]
    nodes, tris = gpu.build.download(keys[0])
    fused = gpu.motion.fuse(*keys)
    mn, mt = sh.records(nodes, tris)
    assert fused.info.tolist() == [0, len(mn) + len(mt), 0, 0]
    same_records(gpu, fused, mn, mt)
    # another topology with the same record counts: the LBVH of key 1 at max_leaf 1
    a, b = (gpu.build.build_bvh2(v, sh.ix, max_leaf=1) for v in (sh.v0, sh.v1))
    assert (a.num_nodes, a.num_tris) == (b.num_nodes, b.num_tris)
    assert gpu.build.download(a)[0]["child"].tobytes() != gpu.build.download(b)[0]["child"].tobytes()
    with pytest.raises(gpu.build.BuildError, match="malformed hierarchy"):
        gpu.motion.fuse(a, b)
    flagged = gpu.motion.fuse(a, b, check=False)
    model = MB.fuse(*gpu.build.download(a), *gpu.build.download(b))
    assert flagged.info.tolist() == model[2].tolist() and model[2][2] == MB.BAD_TOPOLOGY
    same_records(gpu, flagged, model[0], model[1])          # every record took key 0's words


# ---- 3. build flags ---------------------------------------------------------------------------------------------------------------------
def test_build_flags(gpu, shapes):
    sh = shapes[1]
    bvh = gpu.build.build_bvh2(sh.v0, sh.ix, max_leaf=2)
    nodes, tris = gpu.build.download(bvh)
    bad_ix = sh.ix.copy(); bad_ix[7, 1] = len(sh.v0)
    nan1 = sh.v1.copy(); nan1[9, 2] = np.nan
    inf0 = sh.v0.copy(); inf0[100, 0] = np.inf
    for v0, v1, ix, flag, word in ((sh.v0, sh.v1, bad_ix, gpu.build.BAD_INDEX, "vertex index"),
                                   (sh.v0, nan1, sh.ix, gpu.build.NON_FINITE, "non-finite"),
                                   (inf0, sh.v1, sh.ix, gpu.build.NON_FINITE, "non-finite"),
                                   (sh.v0, nan1, bad_ix, gpu.build.BAD_INDEX | gpu.build.NON_FINITE, "vertex index")):
        model = MB.build(nodes, tris, v0, v1, ix)[2]
        assert model[2] == flag
        with pytest.raises(gpu.build.BuildError, match=word):
            gpu.motion.build_motion_bvh2(bvh, v0, v1, ix)
        got = gpu.motion.build_motion_bvh2(bvh, v0, v1, ix, check=False)
        assert got.info.tolist() == model.tolist(), (got.info, model)
    with pytest.raises(ValueError):
        gpu.motion.build_motion_bvh2(bvh, sh.v0, sh.v1[:-1], sh.ix)
    # the synchronous C entry: RODENT_BUILD_ERR_INPUT on a flag, RODENT_BUILD_OK and the info words on a sound call
    t = gpu.torch
    dev = [t.from_numpy(a).cuda() for a in (sh.v0, sh.v1, nan1, sh.ix)]
    out_n = t.empty(len(nodes) * F.MOTION_NODE2.itemsize, dtype=t.uint8, device="cuda")
    out_t = t.empty(len(tris) * F.MOTION_TRI1.itemsize, dtype=t.uint8, device="cuda")
    info = (C.c_int32 * 4)()
    t.cuda.synchronize()
    for v1, rc, words in ((dev[1], 0, [len(nodes), len(nodes) + len(tris), 0, len(nodes)]),
                          (dev[2], -7, [len(nodes), len(nodes) + len(tris), gpu.build.NON_FINITE, len(nodes)])):
        got = gpu.abi.lib().rodent_hip_build_motion_bvh2_tri1_sync(0, dev[0].data_ptr(), v1.data_ptr(), len(sh.v0), dev[3].data_ptr(),
                                                                  len(sh.ix), bvh.nodes.data_ptr(), len(nodes), bvh.tris.data_ptr(),
                                                                  len(tris), out_n.data_ptr(), out_t.data_ptr(), info)
        assert got == rc and list(info) == words


# ---- 4. trace ---------------------------------------------------------------------------------------------------------------------------
CLASSES = [("cornell", "primary"), ("cornell", "random"), ("cornell", "edge"), ("soup", "segments")]


@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name,cls", CLASSES)
def test_trace_equals_the_model(gpu, placed, expected, name, cls, any_hit):
    mbvh = placed[name][2]
    rays, times, m_hits = expected[(name, cls, any_hit)]
    assert len(set(times.view("<u4").tolist())) == 16
    t = gpu.torch
    rays_dev, times_dev = gpu.abi.to_device(rays), t.from_numpy(times).cuda()
    for count in COUNTS + (len(rays),):
        hits = gpu.motion.trace_motion(mbvh, rays[:count], times[:count], any_hit)
        assert hits.tobytes() == m_hits[:count].tobytes(), (name, cls, any_hit, count, "sync")
        hits_dev = t.full((count * F.HIT1.itemsize,), 0xA5, dtype=t.uint8, device="cuda")
        gpu.motion.trace_motion_async(mbvh, rays_dev, times_dev, hits_dev, count, any_hit)
        gpu.abi.check_errors(0)
        assert gpu.abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits[:count].tobytes(), (name, cls, any_hit, count, "async")
    on = MB.traced(times)
    assert (m_hits["tri_id"][on] >= 0).mean() >= 0.25 and (m_hits["tri_id"][~on] == -1).all()


# ---- 5. static anchor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [0, 1])
def test_times_zero_and_one_equal_the_static_trace(gpu, oracle, placed, key):
    for name, (sh, _, mbvh, mn, mt) in placed.items():
        static = gpu.build.refit_bvh2(gpu.build.build_bvh2(sh.v0, sh.ix, max_leaf=2, treelet_passes=2), (sh.v0, sh.v1)[key], sh.ix)
        assert gpu.build.download(static)[0]["child"].tobytes() == mn["child"].tobytes()
        tris = MB.at_time(mn, mt, F32(key))[1]
        for cls, rays in sh.rays.items():
            moving = gpu.motion.trace_motion(mbvh, rays, np.full(len(rays), key, F32))
            still = gpu.abi.traverse(static, rays, variant=0)
            assert np.array_equal(moving["t"], still["t"]), (name, cls)
            brute, second = oracle.brute_force(tris, rays)
            clear = (brute["tri_id"] < 0) | (second != brute["t"])
            assert clear.mean() > 0.5
            assert np.array_equal(moving["tri_id"][clear], still["tri_id"][clear]), (name, cls)
            assert (moving["tri_id"] >= 0).mean() >= 0.25


# ---- 6. stack ---------------------------------------------------------------------------------------------------------------------------
def chain_records(depth, levels):
    """The model's fuse of conftest.chain_bvh2(depth) at two keys, key 1 the chain shifted by 3 along z, each under `levels` padding
    nodes.  (The refit would retighten the chain's artificial boxes, so these records bypass the build.)"""
    keys = [chain_bvh2(depth, z0) for z0 in (200.0, 203.0)]
    (n0, t0), (n1, t1) = [(pad_bvh2_depth(n, levels) if levels else n, t) for n, t in keys]
    mn, mt, info = MB.fuse(n0, t0, n1, t1)
    assert info[2] == 0
    return mn, mt


def chain_rays(n):
    rng = np.random.default_rng(n)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[:, 2] = -1.0
    return F.make_rays(org, np.tile(F32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 1000.0)


@pytest.fixture(scope="module")
def chains(oracle):
    """((records with a peak of 63, model hits), records with a peak of 64, rays, times); each peak asserted with oracle.ray_depths."""
    rays = chain_rays(70)
    times = F32([0.0, 1.0, 0.5, 0.25])[np.arange(70) % 4]
    own = MB.peak(oracle, *chain_records(40, 0), rays, times)
    assert own.min() == own.max() >= 40
    levels = 63 - int(own[0])
    fits = chain_records(40, levels)
    assert (MB.peak(oracle, *fits, rays, times) == 63).all()
    deep = chain_records(40, levels + 1)
    with pytest.raises(RuntimeError, match="stack overflow"):           # one padding node more: 64, which the oracle refuses too
        MB.peak(oracle, *deep, rays, times)
    hits = MB.trace(oracle, *fits, rays, times)
    assert (hits["tri_id"] == 0).all() and len(set(hits["t"].tolist())) == 4      # triangle 0 at z0 + 3 t
    return (fits, hits), deep, rays, times


def test_stack_at_the_limit_and_beyond(gpu, chains):
    (fits, m_hits), deep, rays, times = chains
    t, abi, motion = gpu.torch, gpu.abi, gpu.motion
    ok, over = motion.upload(*fits), motion.upload(*deep)
    assert motion.trace_motion(ok, rays, times).tobytes() == m_hits.tobytes()      # the synchronous entry on the sound case only
    stream = t.cuda.Stream()
    rays_dev, times_dev = abi.to_device(rays), t.from_numpy(times).cuda()
    hits_dev = t.zeros(len(rays) * F.HIT1.itemsize, dtype=t.uint8, device="cuda")
    t.cuda.synchronize()
    motion.trace_motion_async(ok, rays_dev, times_dev, hits_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes()
    # a peak of 64: the flag, and nothing else
    motion.trace_motion_async(over, rays_dev, times_dev, hits_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 1
    # the next sound launch on the stream is clean
    hits_dev.zero_()
    t.cuda.synchronize()
    motion.trace_motion_async(ok, rays_dev, times_dev, hits_dev, len(rays), False, stream)
    assert abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream)) == 0
    assert abi.from_device(hits_dev, F.HIT1).tobytes() == m_hits.tobytes()
    abi.check_errors(0)            # the default stream's context is the one used last again


# ---- 7. time rule -----------------------------------------------------------------------------------------------------------------------
def test_refused_times_store_miss_records_beside_traced_neighbours(gpu, oracle, placed):
    sh, _, mbvh, mn, mt = placed["cornell"]
    rays = sh.rays["primary"][2016:2080].copy()                            # one wave of rays from the middle of the image
    rays["tmax"] = np.arange(64, dtype=F32) + 100.0                        # a tmax of its own per ray: the miss record returns it
    for shift in range(2):
        times = np.where((np.arange(64) + shift) % 2 == 0, F32(0.5), np.resize(X.REFUSED, 64)).astype(F32)
        hits = gpu.motion.trace_motion(mbvh, rays, times)
        off = ~MB.traced(times)
        assert off.sum() == 32
        miss = np.zeros(32, F.HIT1); miss["tri_id"], miss["t"] = -1, rays["tmax"][off]
        assert hits[off].tobytes() == miss.tobytes()
        model = MB.trace(oracle, mn, mt, rays, times)
        assert hits.tobytes() == model.tobytes() and (hits["tri_id"][~off] >= 0).mean() > 0.5
