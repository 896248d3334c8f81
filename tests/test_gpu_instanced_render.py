"""Instanced scenes through the renderer (include/rodent_render.h, "instanced scenes") against tests/instanced_scene_model.py: the
derived tables byte for byte, the stream traversal kernels over the two-level hierarchy ray by ray, the instanced shader vertex by
vertex against the flat oracle on the baked scene, whole frames, the options in effect and the refusals."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import instance_model as M
import instanced_scene_model as IM
import shade_fixtures as SF
from conftest import GOLDEN
from rodent_amd import formats as F, instances as I, scene as S

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = IM.W, IM.H, IM.SPP, IM.MAXLEN


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("instanced"))
    scene = I.concat_scenes(objects)
    transforms, ids = IM.placements()
    return SimpleScene(scene, scene.ranges, transforms, ids, objects[0], IM.object_bvhs(scene, scene.ranges))


class SimpleScene:
    def __init__(self, scene, ranges, transforms, ids, cornell, hierarchy):
        self.scene, self.ranges, self.transforms, self.ids = scene, ranges, transforms, ids
        self.cornell, self.hierarchy = cornell, hierarchy


@pytest.fixture(scope="module")
def cam():
    return S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)


@pytest.fixture(scope="module")
def model(parts, oracle, cam):
    """The model's frame of the test scene, computed once: film, counts, and every ray and vertex it walked."""
    return IM.frame(parts.scene, parts.ranges, parts.transforms, parts.ids, parts.hierarchy, cam, 0, SPP, MAXLEN, W, H)


@contextlib.contextmanager
def rendering(R, parts, spp=SPP, transforms=None, **kw):
    inst = (parts.ranges, parts.transforms if transforms is None else transforms, parts.ids)
    r = R.Renderer(parts.scene, W, H, spp, MAXLEN, instances=inst, **kw)
    try:
        yield r
    finally:
        r.close()


def streams(R, cap):
    l = R.stage_lib()
    p, q, s = R.PrimaryStream(), R.PrimaryStream(), R.SecondaryStream()
    l.rodent_gpu_get_first_primary_stream(0, C.byref(p), cap)
    l.rodent_gpu_get_second_primary_stream(0, C.byref(q), cap)
    l.rodent_gpu_get_secondary_stream(0, C.byref(s), cap)
    return l, p, q, s


def expected_tables(parts, transforms):
    nodes, tris, table = parts.hierarchy
    tlas, inst, info = IM.tlas_of(nodes, table, transforms, parts.ids)
    return {"tlas_nodes": tlas, "instances": inst, "slot_of": IM.slot_of(inst), "bases": IM.bases(parts.ranges, parts.ids),
            "lights": IM.world_lights(parts.scene.lights, parts.ranges, transforms, parts.ids),
            "light_owner": IM.light_owner(parts.ranges, parts.ids), "objects": table, "tlas_info": info}


def assert_tables(got, want, what):
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: `{name}` differs from the model"


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def test_tables_equal_the_model_after_creation_and_after_moves(R, parts, cam):
    import torch
    moved, _ = IM.placements(moved=True)
    other = moved.copy(); other[1:, 3] += np.float32(0.125)
    with rendering(R, parts) as r:
        assert r.transforms_status() == (0, expected_tables(parts, parts.transforms)["tlas_info"].tolist())
        nodes, tris = r.scene_bvh()
        assert nodes.tobytes() == parts.hierarchy[0].tobytes() and tris.tobytes() == parts.hierarchy[1].tobytes()
        assert_tables(r.instance_tables(), expected_tables(parts, parts.transforms), "after creation")
        d = torch.from_numpy(moved).cuda()
        r.set_transforms(d)
        assert r.transforms_status()[0] == 0
        after_move = r.instance_tables()
        assert_tables(after_move, expected_tables(parts, moved), "after set_transforms")
        assert np.array_equal(after_move["descs"]["object_to_world"], moved) and np.array_equal(after_move["descs"]["object"], parts.ids)
        assert np.array_equal(after_move["descs"]["instance_id"], np.arange(len(moved)))
        # two moves on two streams, no check in between (nothing waits): the frame behind them sees the second one
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r.set_transforms(torch.from_numpy(other).cuda(), stream=s1, check=False)
        r.set_transforms(d, stream=s2, check=False)
        r.render(cam, 0)
        film_moved = r.film()
        assert r.transforms_status()[0] == 0
        assert_tables(r.instance_tables(), expected_tables(parts, moved), "after two moves on two streams")
    with rendering(R, parts, transforms=moved) as r:
        fresh = r.instance_tables()
        assert_tables(fresh, expected_tables(parts, moved), "created with the moved matrices")
        for name in after_move:
            assert fresh[name].tobytes() == after_move[name].tobytes(), name
        r.render(cam, 0)
        assert np.allclose(r.film(), film_moved, rtol=FILM_RTOL, atol=FILM_ATOL) and film_moved.mean() > 0.02


# ---- traversal --------------------------------------------------------------------------------------------------------------------------
def crafted_rays(parts):
    """Edge rays: a miss that leaves the scene, rays through the coincident pair of cubes (equal t in two instances), rays at the first
    cube whose tmax ends inside it, in front of it and behind it."""
    t = parts.transforms.reshape(-1, 3, 4).astype(np.float64)
    pair, cube = t[3, :, 3], t[1, :, 3]
    org, d, tmax = [], [], []
    for k in range(8):
        org.append((0.0, 1.0, 2.7)); d.append((0.3 * k, 5.0 + k, 1.0)); tmax.append(SF.FLT_MAX_REF)          # up and out of the open front
    for k in range(16):
        o = np.array([0.4 * np.cos(k), 1.0 + 0.05 * k, 2.5])
        org.append(o); d.append(pair + 0.02 * np.array([np.sin(3 * k), np.cos(5 * k), 0]) - o); tmax.append(SF.FLT_MAX_REF)
    for k, reach in enumerate((0.5, 0.9, 0.97, 1.0, 1.03, 1.1, 1.5, 3.0)):
        o = np.array([-0.2 + 0.05 * k, 0.9, 2.6])
        org.append(o); d.append(cube - o); tmax.append(reach)                                              # t = 1 is the cube's centre
    return F.make_rays(np.float32(org), np.float32(d), 0.0, np.float32(tmax))


def expected_hit_rows(parts, rays, hits, ids, slot_of):
    """Rows geom, prim, t, u, v (uint32 words) and the slot array the closest-hit pass must leave for these model answers."""
    n = len(rays)
    hit = hits["tri_id"] >= 0
    b = IM.bases(parts.ranges, parts.ids)
    gprim = np.where(hit, b[np.maximum(ids, 0), 0] + hits["tri_id"], 0)
    rows = np.zeros((5, n), "<u4")
    rows[0] = np.where(hit, parts.scene.indices[gprim, 3], len(parts.scene.materials)).astype("<i4").view("<u4")
    rows[1] = hits["tri_id"].astype("<i4").view("<u4")
    rows[2] = np.where(hit, SF.bits(hits["t"]), SF.bits(rays["tmax"]))
    rows[3] = np.where(hit, SF.bits(hits["u"]), 0); rows[4] = np.where(hit, SF.bits(hits["v"]), 0)
    return rows, np.where(hit, slot_of[np.maximum(ids, 0)], -1).astype("<i4")


def primary_slab(stream, rays, ids):
    s = SF.sentinel(stream, SF.P_ROWS)
    n = len(rays)
    s[SF.ID, :n] = np.asarray(ids, "<i4").view("<u4")
    s[SF.ORG, :n] = SF.bits(rays["org"].T); s[SF.DIR, :n] = SF.bits(rays["dir"].T)
    s[SF.TMIN, :n] = SF.bits(rays["tmin"]); s[SF.TMAX, :n] = SF.bits(rays["tmax"])
    return s


def test_traversal_equals_the_model_ray_by_ray(R, parts, oracle, model):
    nodes, tris, table = parts.hierarchy
    edge = crafted_rays(parts)
    edge_hits, edge_ids = M.trace(oracle, model.tlas, model.instances, nodes, tris, edge)
    # (the inputs are what they were made to be: misses, both cubes of the pair, a tmax in front of the cube and one inside it)
    assert (edge_hits["tri_id"][:8] < 0).all() and set(edge_ids[8:24]) == {3, 4} and (edge_hits["tri_id"][24:26] < 0).all() \
        and (edge_ids[26:] == 1).all()
    # camera rays, every bounce ray and the crafted rays in ONE stream of a few thousand rays: several workgroups, a last partial wave
    take = [(r[:1500], h[:1500], i[:1500]) for r, _, h, i in model.primary] + [(edge, edge_hits, edge_ids)]
    rays, hits, ids = (np.concatenate([t[k] for t in take]) for k in range(3))
    n = len(rays) - (len(rays) % 64 == 0)                                  # the last wave is a partial one
    rays, hits, ids = rays[:n], hits[:n], ids[:n]
    assert n > 2048
    slot_of = IM.slot_of(model.instances)
    want_rows, want_slots = expected_hit_rows(parts, rays, hits, ids, slot_of)
    with rendering(R, parts, spp=1) as r:
        l, p, q, s = streams(R, n + 100)
        ptr = r.instance_pointers()
        assert ptr["ray_slot_capacity"] >= n + 100
        g0 = primary_slab(p, rays, np.arange(n) % (W * H))
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
            want = g0.copy()
            if form == "20-byte records":
                flat = want[SF.HIT_ROWS].reshape(-1)                       # the five arrays' memory, as words [5 i, 5 i + 5)
                flat[:5 * n] = want_rows.T.reshape(-1)
                want[SF.HIT_ROWS] = flat.reshape(5, -1)
            else:
                want[SF.HIT_ROWS, :n] = want_rows
            SF.assert_same(got, want, form)
            slots = R.read_stream_array(ptr["ray_slots"], ptr["ray_slot_capacity"], "<i4")
            assert np.array_equal(slots[:n], want_slots) and (slots[n:] == 0x7E7E7E7E).all(), form
        # the shadow pass: one ray per pixel, so the film is one float32 add per channel; dead rays between live ones
        sr = np.concatenate([t[0] for t in model.shadow])[: W * H - 7]
        so = np.concatenate([t[2] for t in model.shadow])[: W * H - 7]
        colour = np.concatenate([t[4] for t in model.shadow])[: W * H - 7]
        m = len(sr)
        pixel = np.arange(m, dtype="<i4")[::-1].copy()
        pixel[5::11] = -1; pixel[64:128] = -1
        s0 = SF.sentinel(s, SF.S_ROWS)
        s0[SF.ID, :m] = pixel.view("<u4")
        s0[SF.ORG, :m] = SF.bits(sr["org"].T); s0[SF.DIR, :m] = SF.bits(sr["dir"].T)
        s0[SF.TMIN, :m] = SF.bits(sr["tmin"]); s0[SF.TMAX, :m] = SF.bits(sr["tmax"])
        s0[SF.S_COLOR, :m] = SF.bits(colour.T)
        lit = (so["tri_id"] < 0) & (pixel >= 0)
        assert lit.sum() > 100 and (~lit & (pixel >= 0)).sum() > 100
        for form in ("hip_traverse_secondary", "hip_traverse_streams"):
            r.clear()
            before = SF.read_film(R)
            SF.write_slab(R, s, s0)
            s.size = m
            if form == "hip_traverse_secondary":
                l.hip_traverse_secondary(0, C.byref(s), None)
            else:
                assert l.hip_traverse_streams(0, None, -1, C.byref(s), None, 0, None) == 0
            assert r.trace_kernel_name() == "k_trace_instanced<true>"
            want_film = before.copy()
            want_film[pixel[lit]] = before[pixel[lit]] + colour[lit] * np.float32(1.0)          # inv_spp = 1
            got_film = SF.read_film(R)
            assert np.array_equal(SF.bits(got_film), SF.bits(want_film)), form
            SF.assert_same(SF.read_slab(R, s, SF.S_ROWS), s0, form + ": the stream is only read")


# ---- shader -----------------------------------------------------------------------------------------------------------------------------
def test_shader_equals_the_flat_oracle_on_the_baked_scene(R, parts, oracle, model):
    """hip_shade and hip_shade_compact on the hits the model's frame walked: what they leave behind equals, bit for bit, the flat
    oracle's shading of the baked scene (shade_fixtures.Expected), with the hit records holding OBJECT-LOCAL prim ids and the per-ray
    slot array naming the instance."""
    baked = model.baked
    n_max = W * H - 36
    per = n_max // len(model.vertices) + 1
    v, inst, local = (np.concatenate([t[k][:per] for t in model.vertices])[:n_max] for k in (0, 2, 3))
    n = len(v)
    classes = set(inst.tolist())
    assert classes >= {0, 1, 2, 5, 6} and classes & {3, 4} and n > 1024 and (v["depth"] >= 2).sum() > 50
    slot_of = IM.slot_of(model.instances)
    ids = (np.arange(n) * 5 + 3) % (W * H)
    assert len(np.unique(ids)) == n
    with rendering(R, parts, spp=1) as r:
        l, p, q, s = streams(R, n + 64)
        cap = SF.slab_cap(p)
        g_flat = SF.slab_of(v, ids, baked, cap)                            # prim = the baked triangle: what the oracle shades
        SF.mark_missed(g_flat, np.arange(7, n, 29), baked)
        g_dev = g_flat.copy()
        hit = g_dev[SF.GEOM, :n].view("<i4") < len(baked.materials)
        g_dev[SF.PRIM, :n] = np.where(hit, local.astype("<i4").view("<u4"), g_dev[SF.PRIM, :n])
        ptr = r.instance_pointers()
        slots = np.full(ptr["ray_slot_capacity"], -1, "<i4")
        slots[:n] = np.where(hit, slot_of[inst], -1)
        s0, q0 = SF.sentinel(s, SF.S_ROWS), SF.sentinel(q, SF.P_ROWS)
        exp = SF.Expected(baked, g_flat, s0, n, MAXLEN)
        want_p = exp.primary.copy(); want_p[SF.PRIM] = g_dev[SF.PRIM]
        assert (exp.shade["emits"] != 0).sum() > 3 and (exp.shade["shadow"] != 0).sum() > 200 and exp.bounce.sum() > 200
        R.write_stream_array(ptr["ray_slots"], slots)
        r.clear()
        before = SF.read_film(R)
        SF.write_slab(R, p, g_dev); SF.write_slab(R, s, s0)
        l.hip_shade(0, C.byref(p), C.byref(s), n, None)
        p1, s1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
        SF.assert_same(p1, want_p, "hip_shade primary")
        SF.assert_same(s1, exp.secondary, "hip_shade secondary")
        film = SF.read_film(R)
        assert np.array_equal(SF.bits(film), SF.bits(exp.film_after(before, 1.0))), "hip_shade film"
        want_q, survivors = SF.compacted(p1, q0, p1[SF.ID].view("<i4")[:n] >= 0)
        for mode in (1, 2):
            r.clear()
            SF.write_slab(R, p, g_dev); SF.write_slab(R, q, q0); SF.write_slab(R, s, s0)
            got = l.hip_shade_compact(0, C.byref(p), C.byref(q), C.byref(s), None, n, mode, 256, None)
            pf, qf, sf = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, q, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
            assert got == survivors == q.size
            SF.assert_same(pf, g_dev, f"mode {mode}: `from`")
            SF.assert_same(sf, s1, f"mode {mode}: secondary")
            if mode == 2:                                                  # blocks arrive in any order: the same records (ids are unique)
                order = lambda a: a[:, np.argsort(a[SF.ID, :got], kind="stable")]
                SF.assert_same(qf[:, got:], want_q[:, got:], "mode 2: `to` behind the new size")
                SF.assert_same(order(qf[:, :got]), order(want_q[:, :got]), "mode 2: `to` as a set")
            else:
                SF.assert_same(qf, want_q, "mode 1: `to`")
            assert np.array_equal(SF.bits(SF.read_film(R)), SF.bits(exp.film_after(before, 1.0))), f"mode {mode}: film"


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("fused_compact", [0, 1, 2])
def test_frame_equals_the_model(R, parts, model, cam, overlap, fused_compact):
    with rendering(R, parts, capacity=4096, overlap=overlap, fused_compact=fused_compact) as r:
        r.render(cam, 0)
        c = r.counters()
        film = r.film()
        assert r.trace_kernel_name() == "k_trace_instanced<true>" and c["iterations"] > 3
    assert (c["primary_rays"], c["shadow_rays"], c["generated"]) == (model.counts[0], model.counts[1], W * H * SPP)
    assert np.allclose(film, model.film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02


def test_tiles_and_hit_record_forms_reproduce_the_frame(R, parts, model, cam):
    with rendering(R, parts, hit_records_aos=0) as r:
        for k in range(3):
            r.render_tiles(cam, 0, 5, k, 3)                                  # 32 rows in tiles of 5: a ragged last tile
        film = r.film()
        r.clear()
        r.render_rows(cam, 0, 0, H)
        c = r.counters()
        assert np.allclose(r.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(model.counts)
    assert np.allclose(film, model.film, rtol=FILM_RTOL, atol=FILM_ATOL)


# ---- options ----------------------------------------------------------------------------------------------------------------------------
def test_options_in_effect_follow_the_scene(R, parts, model, cam):
    asked = dict(mapping="megakernel", trace_persistent=2, trace_refill=(40, 32), sort=1, persist_min_rays=0)
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN, **asked)
    flat_options = flat.options_in_effect()
    flat.render(cam, 0)
    flat_kernel = flat.trace_kernel_name()
    flat.close()
    assert flat_options == {"mapping": "megakernel", "trace_persistent": 2, "trace_refill": (40, 32), "sort": 1}
    with rendering(R, parts, **asked) as r:
        assert r.options_in_effect() == {"mapping": "streaming", "trace_persistent": 0, "trace_refill": (0, 0), "sort": 0}
        r.render(cam, 0)
        c = r.counters()
        assert r.trace_kernel_name() == "k_trace_instanced<true>"
        assert np.allclose(r.film(), model.film, rtol=FILM_RTOL, atol=FILM_ATOL)
        assert (c["primary_rays"], c["shadow_rays"]) == tuple(model.counts)
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN, **asked)
    assert flat.options_in_effect() == flat_options
    flat.render(cam, 0)
    assert flat.trace_kernel_name() == flat_kernel
    flat.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_scene_alone(R, parts, oracle, cam):
    from rodent_amd import abi, gpubuild
    scene, ranges, t, ids = parts.scene, parts.ranges, parts.transforms, parts.ids

    def changed(**kw):
        s = copy.copy(scene)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    def rows(*edits):
        out = ranges.copy()
        for o, col, value in edits:
            out[o, col] = value
        return out
    stolen = scene.light_ids.copy()
    quad = ranges[2, 0]
    stolen[quad] = 0                                                       # the quad's first triangle names the box's light
    far = scene.indices.copy(); far[3, 1] = len(scene.vertices)
    assert 3 < quad < len(scene.indices) - 1
    far_last = scene.indices.copy(); far_last[-1, 1] = len(scene.vertices)
    no_material = scene.indices.copy(); no_material[3, 3] = len(scene.materials)
    no_texture = scene.materials.copy(); no_texture["tex_kd"][0] = len(scene.textures) + 1
    with_bvh = changed(nodes=parts.hierarchy[0], tris=parts.hierarchy[1])
    bad_opt = abi.BuildOptions(9, 0, gpubuild.NODE_COST, gpubuild.TRI_COST)
    cases = [("a hierarchy in the description", R.SCENE_ERR_COUNTS, (with_bvh, ranges, t, ids), None),
             ("no instances", R.SCENE_ERR_COUNTS, (scene, ranges, t[:0], ids[:0]), None),
             ("no objects", R.SCENE_ERR_COUNTS, (scene, ranges[:0], t, ids), None),
             ("a gap between triangle ranges", R.SCENE_ERR_RANGES, (scene, rows((1, 0, ranges[1, 0] + 1)), t, ids), None),
             ("triangle ranges that stop short", R.SCENE_ERR_RANGES, (scene, rows((2, 1, 1)), t, ids), None),
             ("an empty object", R.SCENE_ERR_RANGES, (scene, rows((1, 1, 0)), t, ids), None),
             ("light ranges out of order", R.SCENE_ERR_RANGES, (scene, rows((2, 2, 0)), t, ids), None),
             ("a light of another object", R.SCENE_ERR_LIGHT, (changed(light_ids=stolen), ranges, t, ids), None),
             ("an object index outside the table", R.SCENE_ERR_OBJECT, (scene, ranges, t, np.where(np.arange(7) == 4, 3, ids)), None),
             ("a negative object index", R.SCENE_ERR_OBJECT, (scene, ranges, t, np.where(np.arange(7) == 2, -1, ids)), None),
             ("no light in any instance", R.SCENE_ERR_NO_LIGHT, (scene, ranges, t[1:5], ids[1:5]), None),
             ("max_leaf 9", R.SCENE_ERR_OPTIONS, (scene, ranges, t, ids), bad_opt),
             ("a vertex index outside the table", R.SCENE_ERR_TABLE, (changed(indices=far), ranges, t, ids), None),
             ("a material index outside the table", R.SCENE_ERR_TABLE, (changed(indices=no_material), ranges, t, ids), None),
             ("a material that names a texture outside the table", R.SCENE_ERR_TABLE, (changed(materials=no_texture), ranges, t, ids), None),
             # the order of the table checks: materials and textures, then triangle by triangle its indices and then its light
             ("a missing texture before another object's light", R.SCENE_ERR_TABLE,
              (changed(materials=no_texture, light_ids=stolen), ranges, t, ids), None),
             ("an earlier triangle's index before a later one's light", R.SCENE_ERR_TABLE,
              (changed(indices=far, light_ids=stolen), ranges, t, ids), None),
             ("an earlier triangle's light before a later one's index", R.SCENE_ERR_LIGHT,
              (changed(indices=far_last, light_ids=stolen), ranges, t, ids), None)]
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN)
    flat.render(cam, 0)
    film = flat.film()
    want, _ = oracle.render(parts.cornell, cam, 0, SPP, MAXLEN, W, H)
    assert np.allclose(film, want, rtol=FILM_RTOL, atol=FILM_ATOL)
    for what, status, args, opt in cases:
        assert R.create_instanced(0, *args, opt=opt) == status, what
    flat.clear()
    flat.render(cam, 0)                                                  # the flat scene is still loaded and renders as before
    assert np.allclose(flat.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
    flat.close()
    with pytest.raises(gpubuild.BuildError, match="another object|outside its object"):
        R.Renderer(changed(light_ids=stolen), W, H, SPP, MAXLEN, instances=(ranges, t, ids))
    # a flag raised on the device: a singular matrix at creation destroys what was half built and returns a status ...
    flattened = t.copy(); flattened[2, 0:3] = 0
    assert R.create_instanced(0, scene, ranges, flattened, ids) == R.SCENE_ERR_DEVICE
    assert R.lib().rodent_hip_scene_create_flags(0) == M.BAD_TRANSFORM
    with pytest.raises(gpubuild.BuildError, match="singular"):
        R.Renderer(scene, W, H, SPP, MAXLEN, instances=(ranges, flattened, ids))


def test_a_singular_matrix_through_set_transforms_is_a_status(R, parts):
    import torch
    flattened = parts.transforms.copy(); flattened[2, 0:3] = 0
    from rodent_amd import gpubuild
    with rendering(R, parts) as r:
        r.set_transforms(torch.from_numpy(flattened).cuda(), check=False)
        flags, words = r.transforms_status()
        assert flags == M.BAD_TRANSFORM == words[2]
        with pytest.raises(gpubuild.BuildError, match="singular"):
            r.set_transforms(torch.from_numpy(flattened).cuda())
        r.set_transforms(torch.from_numpy(parts.transforms).cuda())        # a sound rebuild: the tables are the model's again
        assert r.transforms_status()[0] == 0
        assert_tables(r.instance_tables(), expected_tables(parts, parts.transforms), "after a sound rebuild")
