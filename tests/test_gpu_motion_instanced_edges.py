"""Moving instances at edge rays, edge keys, edge times and stack limits (the section "moving instances" of include/rodent_instances.h),
against tests/motion_instance_model.py on the inputs of tests/motion_instance_edge_fixtures.py (shown not to be vacuous, on the CPU, by
tests/test_motion_instance_edge_fixtures.py).

* build_motion_tlas gives the model's bytes and info words for every top and max_leaf 1 / 2 / 8; the flag boundary of the inverse at
  each endpoint alone (2^-127 builds; 2^-128 at M0 only, or at M1 only, raises BAD_TRANSFORM and nothing else);
* every ray class on every top it is meant for, closest and any hit, whole and cut to 1 / 63 / 64 / 65 rays, with and without the
  instance-id array, into buffers filled with 0xFF that reach past the launch: Hit1 bytes and instance ids are the model's, nothing
  past `count` is written.  For any hit, rays with a NaN in any input word are compared by hit / no hit only
  (tests/test_gpu_parity.py::test_special_tmin_tmax_values' convention), chosen by the INPUT bits;
* static anchor: on `static_pairs` with all times 0, then 1, then -0, records and ids equal k_instanced over build_tlas(M0) byte for
  byte, for every class (the CPU test shows that the models say so, and what t = -0 does to a -0 entry);
* the three overflow checks of the one 64-entry stack from both sides of P + 2 = 64, on the asynchronous entry with
  rodent_hip_check_errors only (the synchronous entries abort() on the flag by contract); the layout that would overflow if its
  instance were entered raises no flag at times that skip it.
"""
import ctypes as C

import numpy as np
import pytest

import instance_edge_fixtures as E
import instance_model as M
import motion_instance_edge_fixtures as Y
import motion_instance_model as MM
from rodent_amd import formats as F
from test_gpu_motion_instances import same_tlas, upload_tlas

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = (1, 63, 64, 65)
TAIL = 64


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
def objects(gi, block):
    return gi.pack_objects([block, M.flat_object()])


def device_tlas(gi, objects, sc):
    return gi.build_motion_tlas(objects, sc.top.t0, sc.top.t1, sc.top.obj, sc.top.ids, sc.max_leaf)


def filled(count, dtype_bytes):
    import torch
    return torch.full(((count + TAIL) * dtype_bytes,), 0xFF, dtype=torch.uint8, device="cuda")


# ---- TLAS bytes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", Y.MAX_LEAVES)
@pytest.mark.parametrize("top", sorted(Y.TOPS))
def test_tlas_bytes_equal_the_model(gi, objects, block, top, max_leaf):
    sc = Y.scene(block, top, max_leaf)
    assert sc.info[2] == 0
    same_tlas(gi, device_tlas(gi, objects, sc), (sc.tlas, sc.inst, sc.info))


def test_flag_boundary_of_the_inverse_at_each_endpoint(gi, objects, block):
    from rodent_amd import gpubuild
    nodes, _, table = M.pack([block, M.flat_object()])
    sound, bad = E.place(np.eye(3) * 2.0 ** -127)[None], E.place(np.eye(3) * 2.0 ** -128)[None]
    for m0, m1 in ((sound, sound), (bad, sound), (sound, bad)):
        model = MM.build_motion_tlas(nodes, table, MM.descriptors(m0, m1, [0], [3]), 1)
        assert model[2][2] == (0 if m0 is m1 else M.BAD_TRANSFORM)
        if model[2][2]:
            with pytest.raises(gpubuild.BuildError) as refused:
                gi.build_motion_tlas(objects, m0, m1, [0], [3])
            assert "transform" in str(refused.value) and "object index" not in str(refused.value)     # BAD_TRANSFORM and nothing else
        else:
            same_tlas(gi, gi.build_motion_tlas(objects, m0, m1, [0], [3]), model)


# ---- trace parity -----------------------------------------------------------------------------------------------------------------------
def launch(gi, objects, tlas, rays_dev, times_dev, count, any_hit, with_ids, stream=None):
    """(hits, ids or None, whether the bytes past `count` stayed as they were) of one asynchronous launch into 0xFF-filled buffers."""
    import torch
    from rodent_amd import abi
    hits_dev = filled(count, F.HIT1.itemsize)
    ids_dev = filled(count, 4).view(torch.int32) if with_ids else None
    torch.cuda.synchronize()
    gi.trace_motion_async(objects, tlas, rays_dev, times_dev, hits_dev, ids_dev, count, any_hit, stream)
    flag = abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    raw = hits_dev.cpu().numpy()
    untouched = bool((raw[count * F.HIT1.itemsize:] == 0xFF).all())
    ids = None
    if with_ids:
        raw_ids = ids_dev.cpu().numpy()
        ids, untouched = raw_ids[:count], untouched and bool((raw_ids[count:] == -1).all())
    return flag, raw[: count * F.HIT1.itemsize].view(F.HIT1), ids, untouched


def assert_same(what, hits, ids, m_hits, m_ids, loose):
    strict = ~loose
    differ = (hits.view("<u4").reshape(-1, 4) != m_hits.view("<u4").reshape(-1, 4)).any(1) & strict
    assert not differ.any(), (what, int(np.flatnonzero(differ)[0]), hits[differ][:1], m_hits[differ][:1])
    assert np.array_equal(hits["tri_id"][loose] >= 0, m_hits["tri_id"][loose] >= 0), what
    if ids is not None:
        assert np.array_equal(ids[strict], m_ids[strict]), what
        assert np.array_equal(ids[loose] >= 0, m_hits["tri_id"][loose] >= 0), what


@pytest.mark.parametrize("top,cls", Y.CASES)
def test_trace_equals_the_model(gi, oracle, objects, block, top, cls):
    import torch
    from rodent_amd import abi
    rays, times = Y.rays_of(oracle, block, top, cls)
    nan_word = E.non_finite(rays)[0]
    rays_dev, times_dev = abi.to_device(rays), torch.from_numpy(times).cuda()
    for max_leaf in Y.MAX_LEAVES:
        sc = Y.scene(block, top, max_leaf)
        tlas = device_tlas(gi, objects, sc)
        for any_hit in (False, True):
            m_hits, m_ids = Y.expect(oracle, block, top, max_leaf, cls, any_hit)
            loose = nan_word if any_hit else np.zeros(len(rays), bool)
            for count in COUNTS + (len(rays),):
                for with_ids in (True, False):
                    what = (top, cls, max_leaf, any_hit, count, with_ids)
                    flag, hits, ids, untouched = launch(gi, objects, tlas, rays_dev, times_dev, count, any_hit, with_ids)
                    assert flag == 0 and untouched, what
                    assert_same(what, hits, ids, m_hits[:count], m_ids[:count], loose[:count])


# ---- static anchor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(Y.CLASSES))
def test_static_pairs_equal_the_static_kernel(gi, oracle, objects, block, cls):
    import torch
    from rodent_amd import abi
    rays, _ = Y.rays_of(oracle, block, "static_pairs", cls)
    rays_dev = abi.to_device(rays)
    nan_word = E.non_finite(rays)[0]
    for max_leaf in Y.MAX_LEAVES:
        sc = Y.scene(block, "static_pairs", max_leaf)
        tlas = device_tlas(gi, objects, sc)
        static = gi.build_tlas(objects, sc.top.t0, sc.top.obj, sc.top.ids, max_leaf)
        for any_hit in (False, True):
            hits_dev, ids_dev = filled(len(rays), F.HIT1.itemsize), filled(len(rays), 4).view(torch.int32)
            gi.trace_async(objects, static, rays_dev, hits_dev, ids_dev, len(rays), any_hit)
            abi.check_errors(0)
            s_hits, s_ids = abi.from_device(hits_dev, F.HIT1)[: len(rays)], ids_dev.cpu().numpy()[: len(rays)]
            loose = nan_word if any_hit else np.zeros(len(rays), bool)
            for t in F32([0.0, 1.0, -0.0]):
                times_dev = torch.from_numpy(np.full(len(rays), t, F32)).cuda()
                flag, hits, ids, untouched = launch(gi, objects, tlas, rays_dev, times_dev, len(rays), any_hit, True)
                assert flag == 0 and untouched
                assert_same((cls, max_leaf, any_hit, float(t)), hits, ids, s_hits, s_ids, loose)
            assert (s_hits["tri_id"] >= 0).sum() >= 16


# ---- stack limits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Y.STACK_LAYOUTS))
def test_stack_limits(gi, oracle, name):
    """trace_motion_async on a stream of its own and rodent_hip_check_errors: the synchronous entries abort() on the flag by contract."""
    import torch
    from rodent_amd import abi
    obj, t_nodes, inst, rays, times = Y.stack_layout(name)
    nodes, tris, _ = M.pack([obj])
    p = MM.peak(oracle, t_nodes, inst, nodes, tris, rays, times)
    m_hits, m_ids = MM.trace(oracle, t_nodes, inst, nodes, tris, rays, times)
    flagged = bool(p.max() + 2 > 64)
    assert flagged == Y.STACK_LAYOUTS[name][4]
    fits = p + 2 <= 64
    assert fits.sum() >= 16
    objects, tlas = gi.pack_objects([obj]), upload_tlas(gi, t_nodes, inst)
    clean = "chain_22" if Y.STACK_LAYOUTS[name][0] == "chain" else "leaf_62"
    _, c_nodes, c_inst, _, c_times = Y.stack_layout(clean)
    clean_tlas = upload_tlas(gi, c_nodes, c_inst)
    c_hits, c_ids = MM.trace(oracle, c_nodes, c_inst, nodes, tris, rays, c_times)
    stream = torch.cuda.Stream()
    rays_dev = abi.to_device(rays)
    flag, hits, ids, untouched = launch(gi, objects, tlas, rays_dev, torch.from_numpy(times).cuda(), len(rays), False, True, stream)
    assert flag == int(flagged) and untouched
    # every ray whose own P + 2 <= 64 has the model's bytes (in a clean launch: all of them); an overflowing ray's record is undefined
    assert hits[fits].tobytes() == m_hits[fits].tobytes() and np.array_equal(ids[fits], m_ids[fits])
    # the next sound launch on the stream is clean and exact
    flag, hits, ids, untouched = launch(gi, objects, clean_tlas, rays_dev, torch.from_numpy(c_times).cuda(), len(rays), False, True, stream)
    assert flag == 0 and untouched and hits.tobytes() == c_hits.tobytes() and np.array_equal(ids, c_ids)
    abi.check_errors(0)            # the default stream's context is the one used last again, as tests/test_gpu_motion_instances.py leaves it
