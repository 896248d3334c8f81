"""The instanced kernels at edge rays, edge matrices and stack limits (include/rodent_instances.h), against tests/instance_model.py on the
inputs of tests/instance_edge_fixtures.py (shown not to be vacuous, on the CPU, by tests/test_instance_edge_fixtures.py).

Standalone (rodent_amd.instances, k_instanced):
* build_tlas gives the model's bytes for every top level and max_leaf; the flag boundary of the inverse (2^-127 builds, 2^-128 is refused);
* every ray class on every top level it is meant for, closest and any hit, whole and cut to 1 / 63 / 64 / 65 rays, with and without the
  instance-id array, into buffers filled with 0xFF: Hit1 bytes and instance ids are the model's.  For any hit, rays with a NaN in any
  input word are compared by hit / no hit only (tests/test_gpu_parity.py::test_special_tmin_tmax_values' convention), chosen by the
  INPUT bits;
* the three overflow checks of the one 64-entry stack, each from both sides of P + 2 = 64.
Renderer (k_trace_instanced, the scene of tests/test_gpu_instanced_render.py) under the three matrix sets of
instance_edge_fixtures.scene_matrix_sets: the derived tables, and the closest-hit pass and the shadow pass on ray classes a - f of
instance_edge_fixtures.scene_edge_rays, compared class by class.  No frame is rendered with an overflowing stack: the frame calls
abort() on the flag by contract, so that stays out of scope here.
"""
import ctypes as C

import numpy as np
import pytest

import instance_edge_fixtures as E
import instance_model as M
import instanced_scene_model as IM
import shade_fixtures as SF
import test_gpu_instanced_render as TR                             # the scene, the stage entry points and the slab helpers
from rodent_amd import formats as F
from test_gpu_instanced_render import R, parts                     # noqa: F401  (its fixtures, used below)

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65)


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
    return gi.build_tlas(objects, sc.top.transforms, sc.top.obj, sc.top.ids, sc.max_leaf)


def filled(count, dtype_bytes):
    import torch
    return torch.full((max(count, 1) * dtype_bytes,), 0xFF, dtype=torch.uint8, device="cuda")


# ---- TLAS bytes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", E.MAX_LEAVES)
@pytest.mark.parametrize("top", sorted(E.TOPS))
def test_tlas_bytes_equal_the_model(gi, objects, block, top, max_leaf):
    sc = E.scene(block, top, max_leaf)
    assert sc.info[2] == 0
    tlas = device_tlas(gi, objects, sc)
    nodes, inst = gi.download(tlas)
    assert np.array_equal(tlas.info, sc.info), (tlas.info, sc.info)
    assert nodes.tobytes() == sc.tlas.tobytes() and inst.tobytes() == sc.inst.tobytes()


def test_flag_boundary_of_the_inverse(gi, objects, block):
    from rodent_amd import gpubuild
    nodes, _, table = M.pack([block, M.flat_object()])
    for k, flags in E.FLAG_BOUNDARY.items():
        m = E.place(np.eye(3) * 2.0 ** k)[None]
        model = M.build_tlas(nodes, table, M.descriptors(m, [0], [3]), 1)
        assert model[2][2] == flags
        if flags:
            with pytest.raises(gpubuild.BuildError) as refused:
                gi.build_tlas(objects, m, [0], [3])
            assert "transform" in str(refused.value) and "object index" not in str(refused.value)     # BAD_TRANSFORM and nothing else
        else:
            tlas = gi.build_tlas(objects, m, [0], [3])
            got_nodes, got_inst = gi.download(tlas)
            assert np.array_equal(tlas.info, model[2])
            assert got_nodes.tobytes() == model[0].tobytes() and got_inst.tobytes() == model[1].tobytes()


# ---- trace parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top,cls", E.CASES)
def test_trace_equals_the_model(gi, oracle, objects, block, top, cls):
    import torch
    from rodent_amd import abi
    rays = E.rays_of(oracle, block, top, cls)
    nan_word = E.non_finite(rays)[0]
    rays_dev = abi.to_device(rays)
    for max_leaf in E.MAX_LEAVES:
        sc = E.scene(block, top, max_leaf)
        tlas = device_tlas(gi, objects, sc)
        for any_hit in (False, True):
            m_hits, m_ids = E.expect(oracle, block, top, max_leaf, cls, any_hit)
            loose = nan_word if any_hit else np.zeros(len(rays), bool)
            for count in COUNTS + (len(rays),):
                for with_ids in (True, False):
                    hits_dev = filled(count, F.HIT1.itemsize)
                    ids_dev = filled(count, 4).view(torch.int32) if with_ids else None
                    gi.trace_async(objects, tlas, rays_dev, hits_dev, ids_dev, count, any_hit)
                    abi.check_errors(0)
                    hits = abi.from_device(hits_dev, F.HIT1)[:count]
                    what = (top, cls, max_leaf, any_hit, count, with_ids)
                    strict, l = ~loose[:count], loose[:count]
                    differ = (hits.view("<u4").reshape(-1, 4) != m_hits[:count].view("<u4").reshape(-1, 4)).any(1) & strict
                    assert not differ.any(), (what, int(np.flatnonzero(differ)[0]), hits[differ][:1], m_hits[:count][differ][:1])
                    assert np.array_equal(hits["tri_id"][l] >= 0, m_hits["tri_id"][:count][l] >= 0), what
                    if with_ids:
                        ids = ids_dev.cpu().numpy()[:count]
                        assert np.array_equal(ids[strict], m_ids[:count][strict]), what
                        assert np.array_equal(ids[l] >= 0, m_hits["tri_id"][:count][l] >= 0), what


# ---- stack limits -----------------------------------------------------------------------------------------------------------------------
def upload_tlas(gi, nodes, inst):
    from rodent_amd import abi
    return gi.Tlas(abi.to_device(nodes), abi.to_device(inst), len(inst), np.int32([len(nodes), 1, 0, 0]), None, 0)


@pytest.mark.parametrize("name", sorted(E.STACK_LAYOUTS))
def test_stack_limits(gi, oracle, name):
    """trace_async on a stream of its own and rodent_hip_check_errors: the synchronous entries abort() on the flag by contract."""
    import torch
    from rodent_amd import abi
    obj, t_nodes, inst, rays = E.stack_layout(name)
    nodes, tris, _ = M.pack([obj])
    p = M.peak(oracle, t_nodes, inst, nodes, tris, rays)
    m_hits, m_ids = M.trace(oracle, t_nodes, inst, nodes, tris, rays)
    flagged = bool(p.max() + 2 > 64)
    assert flagged == E.STACK_LAYOUTS[name][2]
    fits = p + 2 <= 64
    assert (m_ids[p > 0] == 9).all() and (m_ids[p == 0] == -1).all() and fits.sum() >= 16
    objects, tlas = gi.pack_objects([obj]), upload_tlas(gi, t_nodes, inst)
    clean_nodes = E.stack_layout("leaf_62" if name.startswith("leaf") else "chain_22")[1]
    clean_tlas = upload_tlas(gi, clean_nodes, inst)
    c_hits, c_ids = M.trace(oracle, clean_nodes, inst, nodes, tris, rays)
    stream = torch.cuda.Stream()
    check = lambda: abi.lib().rodent_hip_check_errors(0, C.c_void_p(stream.cuda_stream))
    rays_dev = abi.to_device(rays)

    def launch(which):
        hits_dev, ids_dev = filled(len(rays), F.HIT1.itemsize), filled(len(rays), 4).view(torch.int32)
        torch.cuda.synchronize()
        gi.trace_async(objects, which, rays_dev, hits_dev, ids_dev, len(rays), False, stream)
        flag = check()
        return flag, abi.from_device(hits_dev, F.HIT1), ids_dev.cpu().numpy()
    flag, hits, ids = launch(tlas)
    assert flag == int(flagged)
    # every ray whose own P + 2 <= 64 has the model's bytes (in a clean launch: all of them); an overflowing ray's record is undefined
    assert hits[fits].tobytes() == m_hits[fits].tobytes() and np.array_equal(ids[fits], m_ids[fits])
    # the next launch on the stream is clean and exact
    flag, hits, ids = launch(clean_tlas)
    assert flag == 0 and hits.tobytes() == c_hits.tobytes() and np.array_equal(ids, c_ids)
    abi.check_errors(0)            # the default stream's context is the one used last again, as tests/test_gpu_instances.py leaves it


# ---- the renderer: k_trace_instanced and the derived tables -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_scenes(parts, oracle):
    """Per matrix set: the instance records, the edge rays of all classes in one array, where each class lies in it, and the model's
    answers (closest and any hit)."""
    nodes, tris, table = parts.hierarchy
    assert tuple(parts.ids) == E.SCENE_OBJECT_IDS
    out = {}
    for name, transforms in E.scene_matrix_sets().items():
        tlas, inst, info = IM.tlas_of(nodes, table, transforms, parts.ids)
        assert info[2] == 0
        model = (tlas, inst, nodes, tris)
        classes, _ = E.scene_edge_rays(oracle, name, transforms, model)
        rays = np.concatenate(list(classes.values()))
        rays = rays[: len(rays) - (len(rays) % 64 == 0)]                       # a last partial wave
        spans, start = {}, 0
        for cls, r in classes.items():
            spans[cls] = slice(start, min(start + len(r), len(rays)))
            start += len(r)
        closest, shadow = M.trace(oracle, *model, rays), M.trace(oracle, *model, rays, any_hit=True)
        out[name] = (transforms, inst, rays, spans, closest, shadow)
    return out


def test_renderer_tables_under_edge_matrices(R, parts):
    import torch
    with TR.rendering(R, parts) as r:
        for name, transforms in E.scene_matrix_sets().items():
            r.set_transforms(torch.from_numpy(transforms).cuda())
            assert r.transforms_status()[0] == 0, name
            TR.assert_tables(r.instance_tables(), TR.expected_tables(parts, transforms), name)


@pytest.mark.parametrize("name", sorted(E.SCENE_BOX_TARGET))
def test_renderer_closest_hit_pass_on_edge_rays(R, parts, edge_scenes, name):
    import torch
    transforms, inst, rays, spans, (hits, ids), _ = edge_scenes[name]
    n = len(rays)
    hit = hits["tri_id"] >= 0
    assert sorted(spans) == list(E.SCENE_CLASSES) and all(hit[sp].any() and (~hit[sp]).any() for sp in spans.values())
    want_rows, want_slots = TR.expected_hit_rows(parts, rays, hits, ids, IM.slot_of(inst))
    assert np.array_equal(want_rows[2][~hit], SF.bits(rays["tmax"])[~hit])          # the miss row: tmax bit for bit, NaN payloads too
    with TR.rendering(R, parts, spp=1) as r:
        r.set_transforms(torch.from_numpy(transforms).cuda())
        l, p, q, s = TR.streams(R, n + 100)
        ptr = r.instance_pointers()
        assert ptr["ray_slot_capacity"] >= n + 100
        g0 = TR.primary_slab(p, rays, np.arange(n) % (TR.W * TR.H))
        for form in ("hip_traverse_primary", "five arrays", "20-byte records"):
            SF.write_slab(R, p, g0)
            R.write_stream_array(ptr["ray_slots"], np.full(ptr["ray_slot_capacity"], 0x7E7E7E7E, "<i4"))
            p.size = n
            if form == "hip_traverse_primary":
                l.hip_traverse_primary(0, C.byref(p), None)
            else:
                assert l.hip_traverse_streams(0, C.byref(p), -1, None, None, int(form == "20-byte records"), None) == 0
            assert r.trace_kernel_name() == "k_trace_instanced<false>"
            got = SF.read_slab(R, p, SF.P_ROWS)
            slots = R.read_stream_array(ptr["ray_slots"], ptr["ray_slot_capacity"], "<i4")
            if form == "20-byte records":
                got_rows = got[SF.HIT_ROWS].reshape(-1)[:5 * n].reshape(n, 5).T
            else:
                got_rows = got[SF.HIT_ROWS, :n]
            for cls, sp in spans.items():                                      # class by class, so that a failure names its class
                assert np.array_equal(got_rows[:, sp], want_rows[:, sp]), f"{name}: {form}: hit rows of class {cls}"
                assert np.array_equal(slots[:n][sp], want_slots[sp]), f"{name}: {form}: ray_slots of class {cls}"
            want = g0.copy()
            if form == "20-byte records":
                flat = want[SF.HIT_ROWS].reshape(-1)
                flat[:5 * n] = want_rows.T.reshape(-1)
                want[SF.HIT_ROWS] = flat.reshape(5, -1)
            else:
                want[SF.HIT_ROWS, :n] = want_rows
            SF.assert_same(got, want, f"{name}: {form}")                        # and nothing else was written
            assert (slots[n:] == 0x7E7E7E7E).all(), (name, form)


@pytest.mark.parametrize("name", sorted(E.SCENE_BOX_TARGET))
def test_renderer_shadow_pass_on_edge_rays(R, parts, edge_scenes, name):
    import torch
    transforms, inst, rays, spans, _, (occl, _) = edge_scenes[name]
    m = len(rays)
    assert m <= TR.W * TR.H
    free = occl["tri_id"] < 0
    rng = np.random.default_rng(11)
    colour = (rng.integers(1, 1024, (m, 3)) * 2.0 ** -10).astype(np.float32)     # multiples of 2^-10 below 1: every sum below is exact
    one_each = np.arange(m, dtype="<i4")[::-1].copy()                            # one pixel per ray ...
    one_each[[0, 63]] = -1; one_each[64:128] = -1; one_each[128:256:2] = -1      # ... dead lanes 0 and 63, a whole wave, every second lane
    k = np.arange(m)
    shared = np.where(k < 512, k // 32, 16 + (k - 512) // 64).astype("<i4")      # two pixels per wave, then all 64 lanes on one pixel
    shared[5::17] = -1
    with TR.rendering(R, parts, spp=1) as r:
        r.set_transforms(torch.from_numpy(transforms).cuda())
        l, p, q, s = TR.streams(R, m + 100)
        size_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        for pixel in (one_each, shared):
            s0 = SF.sentinel(s, SF.S_ROWS)
            s0[SF.ID, :m] = pixel.view("<u4")
            s0[SF.ORG, :m] = SF.bits(rays["org"].T); s0[SF.DIR, :m] = SF.bits(rays["dir"].T)
            s0[SF.TMIN, :m] = SF.bits(rays["tmin"]); s0[SF.TMAX, :m] = SF.bits(rays["tmax"])
            s0[SF.S_COLOR, :m] = SF.bits(colour.T)
            lit = free & (pixel >= 0)
            for cls, sp in spans.items():                                      # every class adds to the film and every class is occluded
                assert lit[sp].any() and (~free[sp] & (pixel[sp] >= 0)).any(), cls
            for count in COUNTS + (m,):
                for form in ("hip_traverse_secondary", "hip_traverse_streams", "size on the device"):
                    r.clear()
                    before = SF.read_film(R)
                    SF.write_slab(R, s, s0)
                    s.size = m if form == "size on the device" else count
                    if form == "hip_traverse_secondary":
                        l.hip_traverse_secondary(0, C.byref(s), None)
                    elif form == "hip_traverse_streams":
                        assert l.hip_traverse_streams(0, None, -1, C.byref(s), None, 0, None) == 0
                    else:
                        size_dev.fill_(count)
                        torch.cuda.synchronize()
                        assert l.hip_traverse_streams(0, None, -1, C.byref(s), C.c_void_p(size_dev.data_ptr()), 0, None) == 0
                    assert r.trace_kernel_name() == "k_trace_instanced<true>"
                    want = before.astype(np.float64)
                    np.add.at(want, pixel[:count][lit[:count]], colour[:count][lit[:count]].astype(np.float64))    # inv_spp = 1
                    got = SF.bits(SF.read_film(R))
                    want = SF.bits(want.astype(np.float32))
                    if pixel is one_each:                                      # one pixel per ray: a wrong pixel names its ray's class
                        for cls, sp in spans.items():
                            px = pixel[sp][pixel[sp] >= 0]
                            assert np.array_equal(got[px], want[px]), f"{name}: {form}: {count} rays: film of class {cls}"
                    assert np.array_equal(got, want), (name, form, count)
                    SF.assert_same(SF.read_slab(R, s, SF.S_ROWS), s0, f"{name}: {form}: the stream is only read")
