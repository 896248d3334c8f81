"""Moving instances through the renderer (include/rodent_render.h, "moving instances in the renderer") against
tests/motion_scene_model.py: the derived tables byte for byte, the generation's third draw, both traversal kernels ray by ray with a
time per ray, the moving shader vertex by vertex against the flat oracle on hits baked at their own times, whole frames, the options
in effect and the refusals."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import instance_model as M
import instanced_scene_model as IM
import motion_instance_model as MM
import motion_scene_model as MS
import shade_fixtures as SF
from conftest import GOLDEN
from rodent_amd import instances as I, scene as S

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = MS.W, MS.H, MS.SPP, MS.MAXLEN
F32 = np.float32


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


class Parts:
    pass


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("motion"))
    p = Parts()
    p.scene = I.concat_scenes(objects)
    p.ranges, p.cornell, p.objects = p.scene.ranges, objects[0], objects
    p.t0, p.t1, p.ids = MS.placements()
    p.hierarchy = IM.object_bvhs(p.scene, p.ranges)
    return p


@pytest.fixture(scope="module")
def cam():
    return S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)


def model_frame(parts, cam, shutter):
    return MS.frame(parts.scene, parts.ranges, parts.t0, parts.t1, parts.ids, parts.hierarchy, cam, 0, SPP, MAXLEN, W, H, shutter=shutter)


@pytest.fixture(scope="module")
def model(parts, oracle, cam):
    """The model's frame under the shutter (0, 1), computed once: film, counts, every ray and vertex it walked, with their times."""
    return model_frame(parts, cam, (0.0, 1.0))


@pytest.fixture(scope="module")
def model_mid(parts, oracle, cam):
    return model_frame(parts, cam, (0.25, 0.75))


@contextlib.contextmanager
def rendering(R, parts, spp=SPP, max_path_len=MAXLEN, t0=None, t1=None, **kw):
    motion = (parts.ranges, parts.t0 if t0 is None else t0, parts.t1 if t1 is None else t1, parts.ids)
    r = R.Renderer(parts.scene, W, H, spp, max_path_len, motion=motion, **kw)
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


def expected_tables(parts, t0, t1):
    nodes, tris, table = parts.hierarchy
    tlas, inst, info = MS.tlas_of(nodes, table, t0, t1, parts.ids)
    return {"tlas_nodes": tlas, "instances": inst, "slot_of": IM.slot_of(inst), "bases": IM.bases(parts.ranges, parts.ids),
            "lights": MS.world_lights(parts.scene.lights, parts.ranges, t0, parts.ids),
            "light_owner": IM.light_owner(parts.ranges, parts.ids), "objects": table, "tlas_info": info}


def assert_tables(got, want, what):
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: `{name}` differs from the model"


def moved_placements(parts):
    """The movers somewhere else at both keys; the box and the emitters stay (an emitter's keys stay equal)."""
    m0, m1 = parts.t0.copy(), parts.t1.copy()
    m0[3:, 3] += F32(0.125); m1[3:, 7] += F32(0.0625)
    return m0, m1


# ---- 1. tables --------------------------------------------------------------------------------------------------------------------------
def test_tables_equal_the_model_after_creation_and_after_moves(R, parts, cam):
    import torch
    m0, m1 = moved_placements(parts)
    with rendering(R, parts) as r:
        assert r.transforms_status() == (0, expected_tables(parts, parts.t0, parts.t1)["tlas_info"].tolist())
        nodes, tris = r.scene_bvh()
        assert nodes.tobytes() == parts.hierarchy[0].tobytes() and tris.tobytes() == parts.hierarchy[1].tobytes()
        assert_tables(r.motion_tables(), expected_tables(parts, parts.t0, parts.t1), "after creation")
        d0, d1 = torch.from_numpy(m0).cuda(), torch.from_numpy(m1).cuda()
        r.set_motion_transforms(d0, d1)
        assert r.transforms_status()[0] == 0
        after_move = r.motion_tables()
        assert_tables(after_move, expected_tables(parts, m0, m1), "after set_motion_transforms")
        descs = after_move["descs"]
        assert np.array_equal(descs["object_to_world0"], m0) and np.array_equal(descs["object_to_world1"], m1)
        assert np.array_equal(descs["object"], parts.ids) and np.array_equal(descs["instance_id"], np.arange(len(m0)))
        # two moves on two streams, no check in between (nothing waits): the first with ONE pointer for both keys
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r.set_motion_transforms(d1, d1, stream=s1, check=False)
        r.set_motion_transforms(d0, d1, stream=s2, check=False)
        r.render(cam, 0)
        film_moved = r.film()
        assert r.transforms_status()[0] == 0
        assert_tables(r.motion_tables(), expected_tables(parts, m0, m1), "after two moves on two streams")
        r.set_motion_transforms(d1, d1)
        assert_tables(r.motion_tables(), expected_tables(parts, m1, m1), "both keys from one pointer")
    with rendering(R, parts, t0=m0, t1=m1) as r:
        fresh = r.motion_tables()
        assert_tables(fresh, expected_tables(parts, m0, m1), "created with the moved matrices")
        for name in after_move:
            assert fresh[name].tobytes() == after_move[name].tobytes(), name
        r.render(cam, 0)
        assert np.allclose(r.film(), film_moved, rtol=FILM_RTOL, atol=FILM_ATOL) and film_moved.mean() > 0.02


# ---- 2. generation ----------------------------------------------------------------------------------------------------------------------
def test_generation_draws_the_time_and_stores_it_in_the_depth_word(R, parts, cam, model):
    total = W * H * SPP
    with rendering(R, parts) as r:
        l, p, q, s = streams(R, total + 64)
        st = R.make_settings(cam)
        for size_before, first_ray in ((0, 0), (37, 5)):
            before = SF.sentinel(p, SF.P_ROWS)
            SF.write_slab(R, p, before)
            p.size = size_before
            n = total - first_ray
            l.hip_generate_rays(0, C.byref(p), total + 64, first_ray, n, C.byref(st), 0, W, H, 0, SPP, None)
            assert p.size == size_before + n
            want = SF.generated_slab(cam, 0, W, H, first_ray, n, 0, SPP, before, size_before)      # id, org, dir, tmin, tmax: the flat ones
            dst = slice(size_before, size_before + n)
            rnd, ubits = MS.third_draw(want[SF.RND, dst])
            assert np.array_equal(rnd, model.rnd[first_ray:]) and np.array_equal(ubits, model.ubits[first_ray:])
            want[SF.RND, dst] = rnd
            want[SF.DEPTH, dst] = (ubits.astype("<i4") << 8).view("<u4")
            SF.assert_same(SF.read_slab(R, p, SF.P_ROWS), want, f"first ray {first_ray}")
            assert (want[SF.DEPTH, dst] >> 31 == 0).all() and len(np.unique(ubits)) > n // 2


# ---- 3. traversal -------------------------------------------------------------------------------------------------------------------------
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


def primary_slab(stream, rays, ids, words):
    s = SF.sentinel(stream, SF.P_ROWS)
    n = len(rays)
    s[SF.ID, :n] = np.asarray(ids, "<i4").view("<u4")
    s[SF.ORG, :n] = SF.bits(rays["org"].T); s[SF.DIR, :n] = SF.bits(rays["dir"].T)
    s[SF.TMIN, :n] = SF.bits(rays["tmin"]); s[SF.TMAX, :n] = SF.bits(rays["tmax"])
    s[SF.DEPTH, :n] = np.asarray(words, "<i4").view("<u4")
    return s


def closest_set(parts, oracle, frame, shutter, take):
    """(rays, ubits, depths, hits, instance ids): the first `take` rays of every bounce of the model frame, then the crafted rays at
    their times under `shutter`."""
    nodes, tris, _ = parts.hierarchy
    crafted, cu = MS.crafted_rays(parts.t0)
    ch, ci = MM.trace(oracle, frame.tlas, frame.instances, nodes, tris, crafted, MS.shutter_time(cu, *shutter))
    groups = [(r[:take], u[:take], np.full(len(r[:take]), k), h[:take], i[:take]) for k, (r, _, h, i, u) in enumerate(frame.primary)]
    groups.append((crafted, cu, np.full(len(cu), 3), ch, ci))
    rays, ubits, depth, hits, ids = (np.concatenate([g[k] for g in groups]) for k in range(5))
    n = len(rays) - (len(rays) % 64 == 0)                                  # the last wave is a partial one
    return rays[:n], ubits[:n], depth[:n], hits[:n], ids[:n]


def test_traversal_equals_the_model_ray_by_ray(R, parts, oracle, model, model_mid):
    nodes, tris, table = parts.hierarchy
    slot_of = IM.slot_of(model.instances)
    with rendering(R, parts, spp=1) as r:
        for shutter, frame, take in (((0.0, 1.0), model, 1 << 20), ((0.25, 0.75), model_mid, 400)):
            rays, ubits, depth, hits, ids = closest_set(parts, oracle, frame, shutter, take)
            n = len(rays)
            assert n > (2048 if take > 400 else 512) and set(ids.tolist()) >= {-1, 0, 3, 4, 5, 6}
            want_rows, want_slots = expected_hit_rows(parts, rays, hits, ids, slot_of)
            r.set_shutter(*shutter)
            l, p, q, s = streams(R, n + 100)
            ptr = r.motion_pointers()
            assert ptr["ray_slot_capacity"] >= n + 100
            g0 = primary_slab(p, rays, np.arange(n) % (W * H), R.pack_depth_time(depth, ubits))
            for form in ("hip_traverse_primary", "five arrays", "20-byte records"):
                SF.write_slab(R, p, g0)
                R.write_stream_array(ptr["ray_slots"], np.full(ptr["ray_slot_capacity"], 0x7E7E7E7E, "<i4"))
                p.size = n
                counted = r.counters()
                if form == "hip_traverse_primary":
                    l.hip_traverse_primary(0, C.byref(p), None)
                else:
                    assert l.hip_traverse_streams(0, C.byref(p), -1, None, None, int(form == "20-byte records"), None) == 0
                assert r.trace_kernel_name() == "k_trace_instanced_motion<false>"
                after = r.counters()                                       # (read live: a stage-level call adds to them)
                assert (after["primary_rays"] - counted["primary_rays"], after["shadow_rays"] - counted["shadow_rays"]) == (n, 0), form
                got = SF.read_slab(R, p, SF.P_ROWS)
                want = g0.copy()
                if form == "20-byte records":
                    flat = want[SF.HIT_ROWS].reshape(-1)                   # the five arrays' memory, as words [5 i, 5 i + 5)
                    flat[:5 * n] = want_rows.T.reshape(-1)
                    want[SF.HIT_ROWS] = flat.reshape(5, -1)
                else:
                    want[SF.HIT_ROWS, :n] = want_rows
                SF.assert_same(got, want, f"{shutter} {form}")
                slots = R.read_stream_array(ptr["ray_slots"], ptr["ray_slot_capacity"], "<i4")
                assert np.array_equal(slots[:n], want_slots) and (slots[n:] == 0x7E7E7E7E).all(), form
        # the shadow pass: the time is the float in prim_id; one ray per pixel, so the film is one float32 add per channel; dead rays
        # between live ones; the crafted rays as shadow rays behind the frame's
        crafted, cu = MS.crafted_rays(parts.t0)
        ct = MS.shutter_time(cu, 0.25, 0.75)
        co, _ = MM.trace(oracle, model.tlas, model.instances, nodes, tris, crafted, ct, any_hit=True)
        keep = W * H - 7 - len(crafted)
        sr = np.concatenate([np.concatenate([t[0] for t in model.shadow])[:keep], crafted])
        so = np.concatenate([np.concatenate([t[2] for t in model.shadow])[:keep], co])
        colour = np.concatenate([t[4] for t in model.shadow])[:len(sr)]
        times = np.concatenate([np.concatenate([t[5] for t in model.shadow])[:keep], ct])
        m = len(sr)
        assert m == W * H - 7
        pixel = np.arange(m, dtype="<i4")[::-1].copy()
        pixel[5::11] = -1; pixel[64:128] = -1
        s0 = SF.sentinel(s, SF.S_ROWS)
        s0[SF.ID, :m] = pixel.view("<u4")
        s0[SF.ORG, :m] = SF.bits(sr["org"].T); s0[SF.DIR, :m] = SF.bits(sr["dir"].T)
        s0[SF.TMIN, :m] = SF.bits(sr["tmin"]); s0[SF.TMAX, :m] = SF.bits(sr["tmax"])
        s0[SF.S_PRIM, :m] = SF.bits(times)
        s0[SF.S_COLOR, :m] = SF.bits(colour.T)
        lit = (so["tri_id"] < 0) & (pixel >= 0)
        assert lit.sum() > 100 and (~lit & (pixel >= 0)).sum() > 100
        for form in ("hip_traverse_secondary", "hip_traverse_streams"):
            r.clear()
            before = SF.read_film(R)
            SF.write_slab(R, s, s0)
            s.size = m
            counted = r.counters()
            if form == "hip_traverse_secondary":
                l.hip_traverse_secondary(0, C.byref(s), None)
            else:
                assert l.hip_traverse_streams(0, None, -1, C.byref(s), None, 0, None) == 0
            assert r.trace_kernel_name() == "k_trace_instanced_motion<true>"
            after = r.counters()                                           # the dead rays (pixel -1) are not counted
            assert (after["primary_rays"] - counted["primary_rays"], after["shadow_rays"] - counted["shadow_rays"]) \
                == (0, int((pixel >= 0).sum())), form
            want_film = before.copy()
            want_film[pixel[lit]] = before[pixel[lit]] + colour[lit] * F32(1.0)                   # inv_spp = 1
            assert np.array_equal(SF.bits(SF.read_film(R)), SF.bits(want_film)), form
            SF.assert_same(SF.read_slab(R, s, SF.S_ROWS), s0, form + ": the stream is only read")


# ---- 4. shader --------------------------------------------------------------------------------------------------------------------------
def shader_vertices(parts, frame, n_max):
    """Up to n_max shaded hits of the model frame, from every bounce, the hits outside the box first; baked at their own times."""
    per = n_max // len(frame.vertices) + 1
    picks = []
    for v, _, inst, local, ubits in frame.vertices:
        order = np.argsort(inst == MS.BOX, kind="stable")[:per]
        picks.append((v[order], inst[order], local[order], ubits[order]))
    v, inst, local, ubits = (np.concatenate([p[k] for p in picks])[:n_max] for k in range(4))
    times = MS.shutter_time(ubits, 0.0, 1.0)
    baked = MS.bake_hits(parts.scene, parts.ranges, parts.t0, parts.t1, parts.ids, frame.lights, inst, local, times)
    v = v.copy(); v["prim"] = np.arange(len(v))
    return v, inst, local, ubits, times, baked


def moving_expectation(R, exp, g_dev, depth, ubits, times, n):
    """shade_fixtures.Expected (the flat oracle on the bake) as the MOVING shader leaves the streams: object-local prim ids and packed
    depth words as given, a ray that goes on with (depth + 1) | ubits << 8, a shadow ray with its time's bits in prim_id."""
    want_p, want_s = exp.primary.copy(), exp.secondary.copy()
    want_p[SF.PRIM] = g_dev[SF.PRIM]; want_p[SF.DEPTH] = g_dev[SF.DEPTH]
    ib = np.flatnonzero(exp.bounce)
    want_p[SF.DEPTH, ib] = R.pack_depth_time(depth[ib] + 1, ubits[ib]).view("<u4")
    ish = exp.idx[exp.shade["shadow"] != 0]
    want_s[SF.S_PRIM, ish] = SF.bits(times[ish])
    return want_p, want_s


def test_shader_equals_the_flat_oracle_on_hits_baked_at_their_own_times(R, parts, oracle, model):
    v, inst, local, ubits, times, baked = shader_vertices(parts, model, W * H - 36)
    n = len(v)
    assert set(inst.tolist()) >= {0, 1, 3, 4, 5, 6} and n > 600 and (v["depth"] >= 2).sum() > 50 and len(np.unique(ubits)) > n // 4
    slot_of = IM.slot_of(model.instances)
    ids = (np.arange(n) * 5 + 3) % (W * H)
    assert len(np.unique(ids)) == n
    with rendering(R, parts, spp=1) as r:
        l, p, q, s = streams(R, n + 64)
        cap = SF.slab_cap(p)
        g_flat = SF.slab_of(v, ids, baked, cap)                            # prim = the baked triangle, plain depth: what the oracle shades
        SF.mark_missed(g_flat, np.arange(7, n, 29), baked)
        hit = g_flat[SF.GEOM, :n].view("<i4") < len(baked.materials)

        def device_slab(flat, depth):
            g = flat.copy()
            g[SF.PRIM, :n] = np.where(hit, local.astype("<i4").view("<u4"), g[SF.PRIM, :n])
            g[SF.DEPTH, :n] = R.pack_depth_time(depth, ubits).view("<u4")
            return g
        g_dev = device_slab(g_flat, v["depth"])
        ptr = r.motion_pointers()
        slots = np.full(ptr["ray_slot_capacity"], -1, "<i4")
        slots[:n] = np.where(hit, slot_of[inst], -1)
        s0, q0 = SF.sentinel(s, SF.S_ROWS), SF.sentinel(q, SF.P_ROWS)
        exp = SF.Expected(baked, g_flat, s0, n, MAXLEN)
        want_p, want_s = moving_expectation(R, exp, g_dev, v["depth"], ubits, times, n)
        assert (exp.shade["emits"] != 0).sum() > 3 and (exp.shade["shadow"] != 0).sum() > 200 and exp.bounce.sum() > 200
        R.write_stream_array(ptr["ray_slots"], slots)
        r.clear()
        before = SF.read_film(R)
        SF.write_slab(R, p, g_dev); SF.write_slab(R, s, s0)
        l.hip_shade(0, C.byref(p), C.byref(s), n, None)
        p1, s1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
        SF.assert_same(p1, want_p, "hip_shade primary")
        SF.assert_same(s1, want_s, "hip_shade secondary")
        assert np.array_equal(SF.bits(SF.read_film(R)), SF.bits(exp.film_after(before, 1.0))), "hip_shade film"
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
        # the last depths: asked for 300 vertices the path length in effect is 255; a vertex at depth 254 goes on to 255 with its
        # time bits intact, and a vertex at depth 255 ends there
        r.configure(1, 300)
        assert r.max_path_len() == 255
        for depth_in, goes_on in ((254, True), (255, False)):
            deep = np.full(n, depth_in)
            f2 = g_flat.copy(); f2[SF.DEPTH, :n] = deep.astype("<i4").view("<u4")
            g2 = device_slab(f2, deep)
            exp2 = SF.Expected(baked, f2, s0, n, 255)
            assert (exp2.bounce.sum() > 200) == goes_on and (goes_on or exp2.bounce.sum() == 0)
            want_p2, want_s2 = moving_expectation(R, exp2, g2, deep, ubits, times, n)
            SF.write_slab(R, p, g2); SF.write_slab(R, s, s0)
            l.hip_shade(0, C.byref(p), C.byref(s), n, None)
            p2 = SF.read_slab(R, p, SF.P_ROWS)
            SF.assert_same(p2, want_p2, f"depth {depth_in} primary")
            SF.assert_same(SF.read_slab(R, s, SF.S_ROWS), want_s2, f"depth {depth_in} secondary")
            if goes_on:
                ib = np.flatnonzero(exp2.bounce)
                d, u = R.unpack_depth_time(p2[SF.DEPTH, ib].view("<i4"))
                assert (d == 255).all() and np.array_equal(u, ubits[ib])


# ---- 5. frames --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("fused_compact", [0, 1, 2])
def test_frame_equals_the_model(R, parts, model, cam, overlap, fused_compact):
    with rendering(R, parts, capacity=4096, overlap=overlap, fused_compact=fused_compact) as r:
        r.render(cam, 0)
        c = r.counters()
        film = r.film()
        assert r.trace_kernel_name() == "k_trace_instanced_motion<true>" and c["iterations"] >= 3
    assert (c["primary_rays"], c["shadow_rays"], c["generated"]) == (model.counts[0], model.counts[1], W * H * SPP)
    assert np.allclose(film, model.film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02


def test_tiles_reproduce_the_frame(R, parts, model, cam):
    with rendering(R, parts, capacity=4096, hit_records_aos=0) as r:
        for k in range(3):
            r.render_tiles(cam, 0, 5, k, 3)                                  # 24 rows in tiles of 5: a ragged last tile
        film = r.film()
        r.clear()
        r.render_rows(cam, 0, 0, H)
        c = r.counters()
        assert np.allclose(r.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(model.counts)
    assert np.allclose(film, model.film, rtol=FILM_RTOL, atol=FILM_ATOL)


def test_frame_under_a_narrower_shutter_equals_the_model(R, parts, model, model_mid, cam):
    with rendering(R, parts, capacity=4096, shutter=(0.25, 0.75)) as r:
        assert r.options_in_effect()["shutter"] == (0.25, 0.75)
        r.render(cam, 0)
        c = r.counters()
        film = r.film()
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(model_mid.counts)
    assert np.allclose(film, model_mid.film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02
    assert not np.allclose(model_mid.film, model.film, rtol=1e-3, atol=1e-4)       # (the shutter matters to this scene)


# ---- 6. options and refusals --------------------------------------------------------------------------------------------------------------
def test_options_in_effect_follow_the_scene(R, parts, model, cam):
    asked = dict(mapping="megakernel", trace_persistent=2, trace_refill=(40, 32), sort=1, persist_min_rays=0)
    with rendering(R, parts, max_path_len=300, **asked) as r:
        assert r.options_in_effect() == {"mapping": "streaming", "trace_persistent": 0, "trace_refill": (0, 0), "sort": 0,
                                         "max_path_len": 255, "shutter": (0.0, 1.0)}
        r.set_shutter(0.5, 0.5)
        assert r.options_in_effect()["shutter"] == (0.5, 0.5)
    flat = R.Renderer(parts.cornell, W, H, SPP, 300, **asked)
    assert flat.max_path_len() == 300 and flat.shutter() == (0.0, 1.0)           # (a new renderer starts from the defaults)
    assert flat.options_in_effect() == {"mapping": "megakernel", "trace_persistent": 2, "trace_refill": (40, 32), "sort": 1}
    flat.close()
    with rendering(R, parts, **asked) as r:                                 # path length 4: the model's frame
        r.render(cam, 0)
        c = r.counters()
        assert np.allclose(r.film(), model.film, rtol=FILM_RTOL, atol=FILM_ATOL)
        assert (c["primary_rays"], c["shadow_rays"]) == tuple(model.counts)


def test_refusals_leave_the_loaded_scene_alone(R, parts, oracle, cam):
    from rodent_amd import abi, gpubuild
    scene, ranges, t0, t1, ids = parts.scene, parts.ranges, parts.t0, parts.t1, parts.ids

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
    stolen[ranges[2, 0]] = 0                                                # the quad's first triangle names the box's light
    far = scene.indices.copy(); far[3, 1] = len(scene.vertices)
    with_bvh = changed(nodes=parts.hierarchy[0], tris=parts.hierarchy[1])
    bad_opt = abi.BuildOptions(9, 0, gpubuild.NODE_COST, gpubuild.TRI_COST)
    sliding = t1.copy(); sliding[MS.QUAD_A, 3] = np.nextafter(sliding[MS.QUAD_A, 3], F32(9))      # one ulp is a moving light
    cases = [("an emitter whose keys differ by an ulp", R.SCENE_ERR_MOVING_LIGHT, (scene, ranges, t0, sliding, ids), None),
             ("a hierarchy in the description", R.SCENE_ERR_COUNTS, (with_bvh, ranges, t0, t1, ids), None),
             ("no instances", R.SCENE_ERR_COUNTS, (scene, ranges, t0[:0], t1[:0], ids[:0]), None),
             ("a gap between triangle ranges", R.SCENE_ERR_RANGES, (scene, rows((1, 0, ranges[1, 0] + 1)), t0, t1, ids), None),
             ("a light of another object", R.SCENE_ERR_LIGHT, (changed(light_ids=stolen), ranges, t0, t1, ids), None),
             ("an object index outside the table", R.SCENE_ERR_OBJECT, (scene, ranges, t0, t1, np.where(np.arange(7) == 4, 3, ids)), None),
             ("no light in any instance", R.SCENE_ERR_NO_LIGHT, (scene, ranges, t0[3:], t1[3:], ids[3:]), None),
             ("max_leaf 9", R.SCENE_ERR_OPTIONS, (scene, ranges, t0, t1, ids), bad_opt),
             ("a vertex index outside the table", R.SCENE_ERR_TABLE, (changed(indices=far), ranges, t0, t1, ids), None),
             # the shared refusals come first, in their order: ranges before the moving light
             ("order", R.SCENE_ERR_RANGES, (scene, rows((2, 1, 1)), t0, sliding, ids), None)]
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN)
    flat.render(cam, 0)
    film = flat.film()
    want, _ = oracle.render(parts.cornell, cam, 0, SPP, MAXLEN, W, H)
    assert np.allclose(film, want, rtol=FILM_RTOL, atol=FILM_ATOL)
    for what, status, args, opt in cases:
        assert R.create_motion(0, *args, opt=opt) == status, what
    for open_, close in ((0.5, 0.25), (-0.125, 1.0), (0.0, 1.5), (float("nan"), 1.0), (0.0, float("nan"))):
        assert R.lib().rodent_hip_render_shutter(0, open_, close) == R.SCENE_ERR_SHUTTER == -30
        with pytest.raises(ValueError, match="shutter"):
            R.Renderer(scene, W, H, SPP, MAXLEN, motion=(ranges, t0, t1, ids), shutter=(open_, close))
    assert flat.shutter() == (0.0, 1.0)
    with pytest.raises(ValueError, match="not both"):
        R.Renderer(scene, W, H, SPP, MAXLEN, motion=(ranges, t0, t1, ids), instances=(ranges, t0, ids))
    flat.clear()
    flat.render(cam, 0)                                                  # the flat scene is still loaded and renders as before
    assert np.allclose(flat.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
    flat.close()
    with pytest.raises(gpubuild.BuildError, match="lights stay static"):
        R.Renderer(scene, W, H, SPP, MAXLEN, motion=(ranges, t0, sliding, ids))
    # a flag raised on the device: a singular endpoint at creation destroys what was half built and returns a status
    flattened = t1.copy(); flattened[MS.TUMBLER, 0:3] = 0
    assert R.create_motion(0, scene, ranges, t0, flattened, ids) == R.SCENE_ERR_DEVICE
    assert R.lib().rodent_hip_scene_create_flags(0) == M.BAD_TRANSFORM
    with pytest.raises(gpubuild.BuildError, match="singular"):
        R.Renderer(scene, W, H, SPP, MAXLEN, motion=(ranges, t0, flattened, ids))
    # the static-instance entries see no instanced scene in a moving one
    with rendering(R, parts) as r:
        with pytest.raises(gpubuild.BuildError, match="no instanced scene"):
            r.prepare_deform([1])


def test_a_singular_endpoint_through_set_motion_transforms_is_a_status(R, parts):
    import torch
    from rodent_amd import gpubuild
    flattened = parts.t1.copy(); flattened[MS.TUMBLER, 0:3] = 0
    d0, d1 = torch.from_numpy(parts.t0).cuda(), torch.from_numpy(parts.t1).cuda()
    with rendering(R, parts) as r:
        r.set_motion_transforms(d0, torch.from_numpy(flattened).cuda(), check=False)
        flags, words = r.transforms_status()
        assert flags == M.BAD_TRANSFORM == words[2]
        with pytest.raises(gpubuild.BuildError, match="singular"):
            r.set_motion_transforms(d0, torch.from_numpy(flattened).cuda())
        r.set_motion_transforms(d0, d1)                                    # a sound rebuild: the tables are the model's again
        assert r.transforms_status()[0] == 0
        assert_tables(r.motion_tables(), expected_tables(parts, parts.t0, parts.t1), "after a sound rebuild")


def test_static_instanced_and_flat_scenes_render_their_own_films_afterwards(R, parts, oracle, model, cam):
    with rendering(R, parts, capacity=4096) as r:
        r.render(cam, 0)
        assert np.allclose(r.film(), model.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    transforms, ids = IM.placements()
    static = IM.frame(parts.scene, parts.ranges, transforms, ids, parts.hierarchy, cam, 0, SPP, MAXLEN, W, H)
    r = R.Renderer(parts.scene, W, H, SPP, MAXLEN, instances=(parts.ranges, transforms, ids))
    r.render(cam, 0)
    c = r.counters()
    assert r.trace_kernel_name() == "k_trace_instanced<true>" and r.max_path_len() == MAXLEN
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(static.counts)
    assert np.allclose(r.film(), static.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    r.close()
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN)
    flat.render(cam, 0)
    want, _ = oracle.render(parts.cornell, cam, 0, SPP, MAXLEN, W, H)
    assert np.allclose(flat.film(), want, rtol=FILM_RTOL, atol=FILM_ATOL) and want.mean() > 0.02
    flat.close()
