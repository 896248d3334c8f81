"""Deforming meshes through the renderer (include/rodent_render.h, "deforming meshes in the renderer") against
tests/deforming_scene_model.py: the scene's tables byte for byte after creation and after every kind of update, the generation's third
draw, both traversal kernels ray by ray with a time per ray, the deforming shader vertex by vertex against the flat oracle on hits
baked at their own times, whole frames, the options in effect and the refusals."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import deforming_scene_fixtures as X
import deforming_scene_model as DM
import motion_bvh_model as MB
import shade_fixtures as SF
from conftest import GOLDEN
from motion_bvh_fixtures import REFUSED

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = X.W, X.H, X.SPP, X.MAXLEN
F32 = np.float32
COUNTS = (1, 63, 64, 65)


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    return X.parts(GOLDEN, tmp_path_factory.mktemp("deforming"))


@pytest.fixture(scope="module")
def cam():
    return X.camera()


@pytest.fixture(scope="module")
def model(parts, oracle):
    """The model's frame under the shutter (0, 1), computed once: film, counts, every ray and vertex it walked, with their times."""
    return X.model_frame(parts, (0.0, 1.0))


@pytest.fixture(scope="module")
def model_mid(parts, oracle):
    return X.model_frame(parts, (0.25, 0.75))


@contextlib.contextmanager
def rendering(R, parts, spp=SPP, max_path_len=MAXLEN, vertices1=None, normals1="given", **kw):
    deform = (parts.keys.vertices1 if vertices1 is None else vertices1, parts.keys.normals1 if isinstance(normals1, str) else normals1)
    r = R.Renderer(parts.scene, W, H, spp, max_path_len, deform=deform, **kw)
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


def assert_tables(got, parts, keys, topology, what):
    mn, mt, info = DM.records(topology, keys, parts.scene.indices)
    want = {"vertices0": keys.vertices0, "vertices1": keys.vertices1, "normals0": keys.normals0, "normals1": keys.normals1,
            "motion_nodes": mn, "motion_tris": mt, "lights": np.asarray(parts.scene.lights), "info": info}
    assert info.tolist() == [len(mn), len(mn) + len(mt), 0, len(mn)]
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: `{name}` differs from the model"


# ---- 1. tables --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [(1, 0), (2, 0), (4, 0), (2, 2)], ids=lambda b: f"max_leaf{b[0]}-passes{b[1]}")
def test_tables_equal_the_model_after_creation(R, parts, build):
    from rodent_amd import gpubuild
    with rendering(R, parts, build=build) as r:
        nodes, tris = r.scene_bvh()                                         # the static key-0 hierarchy: the topology of every rebuild
        alone = gpubuild.download(gpubuild.build_bvh2(parts.keys.vertices0, parts.scene.indices, max_leaf=build[0],
                                                      treelet_passes=build[1]))
        assert nodes.tobytes() == alone[0].tobytes() and tris.tobytes() == alone[1].tobytes()
        if build == (2, 0):
            assert nodes.tobytes() == parts.topology[0].tobytes() and tris.tobytes() == parts.topology[1].tobytes()
        assert r.motion_keys_status() == (0, [len(nodes), len(nodes) + len(tris), 0, len(nodes)])
        assert_tables(r.deforming_tables(), parts, parts.keys, (nodes, tris), "after creation")
        ptr = r.scene_table_pointers()
        assert ptr["tri_shade"] == 0 and ptr["top_image"] == 0 and ptr["top_image_large"] == 0


def test_host_smooth_normals_of_key_1_when_none_are_given(R, parts):
    with rendering(R, parts, normals1=None) as r:
        assert_tables(r.deforming_tables(), parts, parts.keys, r.scene_bvh(), "normals1 = None")      # (the fixtures' key 1 is smooth)


def test_tables_equal_the_model_after_updates(R, parts, cam):
    import torch
    m0, m1 = X.moved_keys(parts)
    k = parts.keys
    given = DM.Keys(m0, m1, k.normals1, k.normals0)                         # any normals: the other key's
    smooth = DM.smooth_keys(m0, m1, parts.scene.indices)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with rendering(R, parts) as r:
        topology = r.scene_bvh()
        d0, d1 = dev(m0), dev(m1)
        r.set_motion_keys(d0, d1, dev(given.normals0), dev(given.normals1))
        assert r.motion_keys_status()[0] == 0
        assert_tables(r.deforming_tables(), parts, given, topology, "given normals")
        r.set_motion_keys(d0, d1)
        after = r.deforming_tables()
        assert_tables(after, parts, smooth, topology, "NULL normals")
        again = r.scene_bvh()                                               # the topology was only read
        assert again[0].tobytes() == topology[0].tobytes() and again[1].tobytes() == topology[1].tobytes()
        # two updates on two streams, no check in between (nothing waits): the first with ONE tensor for both keys
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r.set_motion_keys(d1, d1, stream=s1, check=False)
        r.set_motion_keys(d0, d1, stream=s2, check=False)
        r.render(cam, 0)
        film_moved = r.film()
        assert r.motion_keys_status()[0] == 0
        assert_tables(r.deforming_tables(), parts, smooth, topology, "two updates on two streams")
        r.set_motion_keys(d1, d1)
        assert_tables(r.deforming_tables(), parts, DM.smooth_keys(m1, m1, parts.scene.indices), topology, "one tensor for both keys")
        # the scene's own table as vertices0_dev, written in place: nothing is copied
        own = r.motion_key_tensor("vertices0")
        assert own.data_ptr() == r.motion_key_pointers()["vertices0"] == r.scene_table_pointers()["vertices"]
        own.copy_(d0)
        r.set_motion_keys(own, d1)
        assert_tables(r.deforming_tables(), parts, smooth, topology, "the scene's own table as key 0")
    with rendering(R, parts, vertices1=m1, normals1=smooth.normals1) as r:   # (key 0 is the fixtures': only key 1 is comparable)
        fresh = r.deforming_tables()
        assert fresh["vertices1"].tobytes() == after["vertices1"].tobytes() and fresh["normals1"].tobytes() == after["normals1"].tobytes()
    assert film_moved.mean() > 0.02


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
            rnd, ubits = DM.third_draw(want[SF.RND, dst])
            assert np.array_equal(rnd, model.rnd[first_ray:]) and np.array_equal(ubits, model.ubits[first_ray:])
            want[SF.RND, dst] = rnd
            want[SF.DEPTH, dst] = DM.pack(np.zeros(n, np.int64), ubits).view("<u4")
            SF.assert_same(SF.read_slab(R, p, SF.P_ROWS), want, f"first ray {first_ray}")
            assert (want[SF.DEPTH, dst] >> 31 == 0).all() and len(np.unique(ubits)) > n // 2


# ---- 3. traversal -------------------------------------------------------------------------------------------------------------------------
def expected_hit_rows(parts, rays, hits):
    """Rows geom, prim, t, u, v (uint32 words) the closest-hit pass must leave for these model answers."""
    hit = hits["tri_id"] >= 0
    rows = np.zeros((5, len(rays)), "<u4")
    material = np.asarray(parts.scene.indices)[np.maximum(hits["tri_id"], 0), 3]
    rows[0] = np.where(hit, material, len(parts.scene.materials)).astype("<i4").view("<u4")
    rows[1] = hits["tri_id"].astype("<i4").view("<u4")
    rows[2] = np.where(hit, SF.bits(hits["t"]), SF.bits(rays["tmax"]))
    rows[3] = np.where(hit, SF.bits(hits["u"]), 0); rows[4] = np.where(hit, SF.bits(hits["v"]), 0)
    return rows


def primary_slab(stream, rays, ids, words):
    s = SF.sentinel(stream, SF.P_ROWS)
    n = len(rays)
    s[SF.ID, :n] = np.asarray(ids, "<i4").view("<u4")
    s[SF.ORG, :n] = SF.bits(rays["org"].T); s[SF.DIR, :n] = SF.bits(rays["dir"].T)
    s[SF.TMIN, :n] = SF.bits(rays["tmin"]); s[SF.TMAX, :n] = SF.bits(rays["tmax"])
    s[SF.DEPTH, :n] = np.asarray(words, "<i4").view("<u4")
    return s


def closest_set(parts, oracle, frame, shutter, take):
    """(rays, ubits, depths, hits): the seeded rays at their times under `shutter`, then the first `take` rays of every bounce of the
    model frame (camera rays, then bounce rays); the last wave is a partial one."""
    seeded, su = X.seeded_rays(parts)
    sh = MB.trace(oracle, frame.nodes, frame.tris, seeded, DM.shutter_time(su, *shutter))
    groups = [(seeded, su, np.full(len(su), 3), sh)]
    groups += [(r[:take], u[:take], np.full(len(r[:take]), k), h[:take]) for k, (r, _, h, u) in enumerate(frame.primary)]
    rays, ubits, depth, hits = (np.concatenate([g[k] for g in groups]) for k in range(4))
    n = len(rays) - (len(rays) % 64 == 0)
    return rays[:n], ubits[:n], depth[:n], hits[:n]


def test_closest_hit_pass_equals_the_model_ray_by_ray(R, parts, oracle, model, model_mid):
    with rendering(R, parts, spp=1) as r:
        for shutter, frame, take in (((0.0, 1.0), model, 1 << 20), ((0.25, 0.75), model_mid, 300)):
            rays, ubits, depth, hits = closest_set(parts, oracle, frame, shutter, take)
            n = len(rays)
            hit = hits["tri_id"] >= 0
            assert n > (2048 if take > 300 else 512) and n % 64 != 0 and 0.25 <= hit.mean() < 1.0
            assert np.isin(parts.quad_tris, hits["tri_id"]).all() and np.isin(hits["tri_id"], parts.box_tris).sum() > 100
            want_rows = expected_hit_rows(parts, rays, hits)
            r.set_shutter(*shutter)
            l, p, q, s = streams(R, n + 100)
            g0 = primary_slab(p, rays, np.arange(n) % (W * H), R.pack_depth_time(depth, ubits))
            launches = [("hip_traverse_primary", n), ("five arrays", n), ("20-byte records", n)]
            launches += [("hip_traverse_primary", c) for c in COUNTS] if take > 300 else []
            for form, count in launches:
                SF.write_slab(R, p, g0)
                p.size = count
                counted = r.counters()
                if form == "hip_traverse_primary":
                    l.hip_traverse_primary(0, C.byref(p), None)
                else:
                    assert l.hip_traverse_streams(0, C.byref(p), -1, None, None, int(form == "20-byte records"), None) == 0
                assert r.trace_kernel_name() == "k_trace_deforming<false>"
                after = r.counters()                                       # (read live: a stage-level call adds to them)
                assert (after["primary_rays"] - counted["primary_rays"], after["shadow_rays"] - counted["shadow_rays"]) == (count, 0), form
                got = SF.read_slab(R, p, SF.P_ROWS)
                want = g0.copy()
                if form == "20-byte records":
                    flat = want[SF.HIT_ROWS].reshape(-1)                   # the five arrays' memory, as words [5 i, 5 i + 5)
                    flat[:5 * count] = want_rows[:, :count].T.reshape(-1)
                    want[SF.HIT_ROWS] = flat.reshape(5, -1)
                else:
                    want[SF.HIT_ROWS, :count] = want_rows[:, :count]
                SF.assert_same(got, want, f"{shutter} {form} {count}")


def test_shadow_pass_equals_the_model_and_keeps_the_time_rule(R, parts, oracle, model):
    """The time is the float in prim_id; one ray per pixel, so the film is one float32 add per channel; dead rays between live ones;
    the seeded rays as shadow rays behind the frame's; and words outside [0, 1] -- a NaN among them -- beside traced rays in one wave:
    such a ray is not occluded and adds its colour."""
    seeded, su = X.seeded_rays(parts)
    keep = W * H - 7 - len(seeded)
    every = slice(0, 4 * keep, 4)                                          # every fourth shadow ray of the frame: all of the image
    sr = np.concatenate([np.concatenate([t[0] for t in model.shadow])[every], seeded])
    colour = np.concatenate([t[3] for t in model.shadow])[:len(sr)]
    times = np.concatenate([np.concatenate([t[4] for t in model.shadow])[every], DM.shutter_time(su, 0.25, 0.75)])
    refused = np.arange(130, 258, 3)                                        # two waves in which every third ray is refused
    times[refused] = np.resize(REFUSED, len(refused))
    occluded = MB.trace(oracle, model.nodes, model.tris, sr, times, any_hit=True)["tri_id"] >= 0
    at_half = MB.trace(oracle, model.nodes, model.tris, sr[refused], np.full(len(refused), 0.5, F32), any_hit=True)["tri_id"] >= 0
    assert not occluded[refused].any() and at_half.sum() > 5                # (traced at a sound time some of them are occluded)
    m = len(sr)
    assert m == W * H - 7
    pixel = np.arange(m, dtype="<i4")[::-1].copy()
    pixel[5::11] = -1; pixel[64:128] = -1
    with rendering(R, parts, spp=1) as r:
        l, p, q, s = streams(R, m + 100)
        s0 = SF.sentinel(s, SF.S_ROWS)
        s0[SF.ID, :m] = pixel.view("<u4")
        s0[SF.ORG, :m] = SF.bits(sr["org"].T); s0[SF.DIR, :m] = SF.bits(sr["dir"].T)
        s0[SF.TMIN, :m] = SF.bits(sr["tmin"]); s0[SF.TMAX, :m] = SF.bits(sr["tmax"])
        s0[SF.S_PRIM, :m] = SF.bits(times)
        s0[SF.S_COLOR, :m] = SF.bits(colour.T)
        lit = ~occluded & (pixel >= 0)
        assert lit.sum() > 100 and (~lit & (pixel >= 0)).sum() > 100
        for form, count in [("hip_traverse_secondary", m), ("hip_traverse_streams", m)] + [("hip_traverse_secondary", c) for c in COUNTS]:
            r.clear()
            before = SF.read_film(R)
            SF.write_slab(R, s, s0)
            s.size = count
            counted = r.counters()
            if form == "hip_traverse_secondary":
                l.hip_traverse_secondary(0, C.byref(s), None)
            else:
                assert l.hip_traverse_streams(0, None, -1, C.byref(s), None, 0, None) == 0
            assert r.trace_kernel_name() == "k_trace_deforming<true>"
            after = r.counters()                                           # the dead rays (pixel -1) are not counted
            assert (after["primary_rays"] - counted["primary_rays"], after["shadow_rays"] - counted["shadow_rays"]) \
                == (0, int((pixel[:count] >= 0).sum())), (form, count)
            on = lit & (np.arange(m) < count)
            want_film = before.copy()
            want_film[pixel[on]] = before[pixel[on]] + colour[on] * F32(1.0)                     # inv_spp = 1
            assert np.array_equal(SF.bits(SF.read_film(R)), SF.bits(want_film)), (form, count)
            SF.assert_same(SF.read_slab(R, s, SF.S_ROWS), s0, form + ": the stream is only read")


# ---- 4. shader --------------------------------------------------------------------------------------------------------------------------
def shader_vertices(parts, oracle, frame, n_max):
    """Up to n_max shaded hits, baked at their own times under the shutter (0, 1): hits of the seeded rays on the turning quad (both
    sides of its flat time), then from every bounce of the model frame the hits whose result differs under the wrong face-normal rule,
    the hits on the light, the hits on the boxes and the quad, and the rest."""
    seeded, su = X.seeded_rays(parts)
    st = DM.shutter_time(su, 0.0, 1.0)
    sh = MB.trace(oracle, frame.nodes, frame.tris, seeded, st)
    on_quad = np.isin(sh["tri_id"], parts.quad_tris)
    entering = X.quad_entering(parts, frame, seeded[on_quad], sh[on_quad], st[on_quad])
    assert entering.sum() >= 3 and (~entering).sum() >= 3
    picks = [(X.vertices_of_rays(seeded[on_quad], sh[on_quad]), sh["tri_id"][on_quad], su[on_quad])]
    per = (n_max - int(on_quad.sum())) // len(frame.vertices) + 1
    wrong = 0
    for b, (v, _, prims, ubits) in enumerate(frame.vertices):
        differs = X.wrong_rule_differs(parts, frame, b, (0.0, 1.0))
        moving = np.isin(prims, np.concatenate([parts.box_tris, parts.quad_tris]))
        emitter = np.asarray(parts.scene.materials)["emissive"][np.asarray(parts.scene.indices)[prims, 3]] != 0
        order = np.argsort(-(4 * differs.astype(int) + 2 * emitter.astype(int) + moving.astype(int)), kind="stable")[:per]
        wrong += int(differs[order].sum())
        picks.append((v[order], prims[order], ubits[order]))
    assert wrong >= 1, "a hit that tells the wrong face-normal rule from the right one"
    v, prims, ubits = (np.concatenate([p[k] for p in picks])[:n_max] for k in range(3))
    times = DM.shutter_time(ubits, 0.0, 1.0)
    baked = DM.bake_hits(parts.scene, parts.keys, frame.lights, prims, times)
    v = v.copy(); v["prim"] = np.arange(len(v))
    return v, prims, ubits, times, baked


def deforming_expectation(R, exp, g_dev, depth, ubits, times):
    """shade_fixtures.Expected (the flat oracle on the bake) as the DEFORMING shader leaves the streams: the scene's prim ids and packed
    depth words as given, a ray that goes on with (depth + 1) | ubits << 8, a shadow ray with its time's bits in prim_id."""
    want_p, want_s = exp.primary.copy(), exp.secondary.copy()
    want_p[SF.PRIM] = g_dev[SF.PRIM]; want_p[SF.DEPTH] = g_dev[SF.DEPTH]
    ib = np.flatnonzero(exp.bounce)
    want_p[SF.DEPTH, ib] = R.pack_depth_time(depth[ib] + 1, ubits[ib]).view("<u4")
    ish = exp.idx[exp.shade["shadow"] != 0]
    want_s[SF.S_PRIM, ish] = SF.bits(times[ish])
    return want_p, want_s


def test_shader_equals_the_flat_oracle_on_hits_baked_at_their_own_times(R, parts, oracle, model):
    v, prims, ubits, times, baked = shader_vertices(parts, oracle, model, W * H - 36)
    n = len(v)
    assert n > 600 and (v["depth"] >= 2).sum() > 50 and len(np.unique(ubits)) > n // 4
    assert np.isin(prims, parts.box_tris).sum() > 200 and np.isin(prims, parts.quad_tris).sum() > 20
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
            g[SF.PRIM, :n] = np.where(hit, prims.astype("<i4").view("<u4"), g[SF.PRIM, :n])
            g[SF.DEPTH, :n] = R.pack_depth_time(depth, ubits).view("<u4")
            return g
        g_dev = device_slab(g_flat, v["depth"])
        s0, q0 = SF.sentinel(s, SF.S_ROWS), SF.sentinel(q, SF.P_ROWS)
        exp = SF.Expected(baked, g_flat, s0, n, MAXLEN)
        want_p, want_s = deforming_expectation(R, exp, g_dev, v["depth"], ubits, times)
        assert (exp.shade["emits"] != 0).sum() > 3 and (exp.shade["shadow"] != 0).sum() > 200 and exp.bounce.sum() > 200
        r.clear()
        before = SF.read_film(R)
        SF.write_slab(R, p, g_dev); SF.write_slab(R, s, s0)
        l.hip_shade(0, C.byref(p), C.byref(s), n, None)                    # fused_compact 0: in place
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
            want_p2, want_s2 = deforming_expectation(R, exp2, g2, deep, ubits, times)
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
def test_frame_equals_the_model(R, parts, model_mid, cam, overlap, fused_compact):
    with rendering(R, parts, capacity=4096, overlap=overlap, fused_compact=fused_compact, shutter=(0.25, 0.75)) as r:
        r.render(cam, 0)
        c = r.counters()
        film = r.film()
        assert r.trace_kernel_name() == "k_trace_deforming<true>" and c["iterations"] >= 3
    assert (c["primary_rays"], c["shadow_rays"], c["generated"]) == (model_mid.counts[0], model_mid.counts[1], W * H * SPP)
    assert np.allclose(film, model_mid.film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02


def test_rows_and_tiles_reproduce_the_frame(R, parts, model, model_mid, cam):
    with rendering(R, parts, capacity=4096, hit_records_aos=0, shutter=(0.25, 0.75)) as r:
        for k in range(3):
            r.render_tiles(cam, 0, 5, k, 3)                                  # 24 rows in tiles of 5: a ragged last tile
        film = r.film()
        r.clear()
        r.render_rows(cam, 0, 0, H)
        c = r.counters()
        assert np.allclose(r.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
        assert (c["primary_rays"], c["shadow_rays"]) == tuple(model_mid.counts)
        assert np.allclose(film, model_mid.film, rtol=FILM_RTOL, atol=FILM_ATOL)
        r.set_shutter(0.0, 1.0)                                            # the whole interval: another frame
        r.clear()
        r.render(cam, 0)
        c = r.counters()
        assert (c["primary_rays"], c["shadow_rays"]) == tuple(model.counts)
        assert np.allclose(r.film(), model.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    assert not np.allclose(model_mid.film, model.film, rtol=1e-3, atol=1e-4)       # (the shutter matters to this scene)


def test_a_frame_after_set_motion_keys_is_the_model_of_the_new_keys(R, parts, oracle, cam):
    import torch
    m0, m1 = X.moved_keys(parts)
    keys = DM.smooth_keys(m0, m1, parts.scene.indices)
    want = X.model_frame(parts, (0.0, 1.0), keys=keys)
    with rendering(R, parts, capacity=4096) as r:
        r.set_motion_keys(torch.from_numpy(m0).cuda(), torch.from_numpy(m1).cuda(), stream=torch.cuda.Stream(), check=False)
        r.render(cam, 0)                                                    # ordered behind the update, whichever stream that took
        c = r.counters()
        assert r.motion_keys_status()[0] == 0
        assert (c["primary_rays"], c["shadow_rays"]) == tuple(want.counts)
        assert np.allclose(r.film(), want.film, rtol=FILM_RTOL, atol=FILM_ATOL) and want.film.mean() > 0.02


# ---- 6. options and refusals --------------------------------------------------------------------------------------------------------------
def test_options_in_effect_follow_the_scene(R, parts, model, cam):
    asked = dict(mapping="megakernel", trace_persistent=2, trace_refill=(40, 32), sort=1, persist_min_rays=0)
    with rendering(R, parts, max_path_len=300, **asked) as r:
        assert r.options_in_effect() == {"mapping": "streaming", "trace_persistent": 0, "trace_refill": (0, 0), "sort": 0,
                                         "max_path_len": 255, "shutter": (0.0, 1.0)}
        r.set_shutter(0.5, 0.5)
        assert r.options_in_effect()["shutter"] == (0.5, 0.5)
    flat = R.Renderer(parts.scene, W, H, SPP, 300, **asked)
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
    from rodent_amd import formats as F
    whole, k = parts.scene, parts.keys
    v1, n1 = k.vertices1, k.normals1

    def changed(**kw):
        s = copy.copy(whole)
        for name, value in dict(dict(nodes=np.zeros(0, F.NODE2), tris=np.zeros(0, F.TRI1)), **kw).items():
            setattr(s, name, value)
        return s
    scene = changed()                                                       # the description without its hierarchy: what the entry takes
    far = scene.indices.copy(); far[3, 1] = len(scene.vertices)
    with_bvh = changed(nodes=parts.topology[0], tris=parts.topology[1])
    bad_opt = abi.BuildOptions(9, 0, gpubuild.NODE_COST, gpubuild.TRI_COST)
    ix = np.asarray(scene.indices)
    emitter = np.flatnonzero(np.asarray(scene.materials)["emissive"][ix[:, 3]] != 0)[0]
    sliding = v1.copy(); sliding[ix[emitter, 1], 3] = np.nextafter(sliding[ix[emitter, 1], 3], F32(9))     # one ulp, in the fourth word
    cases = [("a NULL table", R.SCENE_ERR_COUNTS, (scene, None, n1), None),
             ("NULL normals", R.SCENE_ERR_COUNTS, (scene, v1, None), None),
             ("a hierarchy in the description", R.SCENE_ERR_COUNTS, (with_bvh, v1, n1), None),
             ("max_leaf 9", R.SCENE_ERR_OPTIONS, (scene, v1, n1), bad_opt),
             ("a vertex index outside the table", R.SCENE_ERR_TABLE, (changed(indices=far), v1, n1), None),
             ("a moved emitter corner", R.SCENE_ERR_MOVING_LIGHT, (scene, sliding, n1), None),
             # in order: counts before options before the table before the moving light
             ("order 1", R.SCENE_ERR_COUNTS, (with_bvh, sliding, n1), bad_opt),
             ("order 2", R.SCENE_ERR_OPTIONS, (changed(indices=far), sliding, n1), bad_opt),
             ("order 3", R.SCENE_ERR_TABLE, (changed(indices=far), sliding, n1), None)]
    flat = R.Renderer(whole, W, H, SPP, MAXLEN)
    flat.render(cam, 0)
    film = flat.film()
    want, _ = oracle.render(whole, cam, 0, SPP, MAXLEN, W, H)
    assert np.allclose(film, want, rtol=FILM_RTOL, atol=FILM_ATOL)
    for what, status, args, opt in cases:
        assert R.create_deforming(0, *args, opt=opt) == status, what
    deform = (v1, n1)
    with pytest.raises(ValueError, match="`deform` or `instances`, not both"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=deform, instances=(np.zeros((1, 4), np.int32), np.zeros((1, 12), F32), [0]))
    with pytest.raises(ValueError, match="`deform` or `motion`, not both"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=deform, motion=(np.zeros((1, 4), np.int32),) + (np.zeros((1, 12), F32),) * 2 + ([0],))
    with pytest.raises(ValueError, match="not gpu_bvh"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=deform, gpu_bvh=2)
    with pytest.raises(ValueError, match="shutter"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=deform, shutter=(0.5, 0.25))
    flat.clear()
    flat.render(cam, 0)                                                  # the flat scene is still loaded and renders as before
    assert np.allclose(flat.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL)
    flat.close()
    with pytest.raises(gpubuild.BuildError, match="lights stay static"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=(sliding, n1))
    # a flag raised on the device: a non-finite coordinate at key 1 destroys what was half built and returns a status
    broken = v1.copy(); broken[parts.tall[3], 1] = np.inf
    assert R.create_deforming(0, scene, broken, n1) == R.SCENE_ERR_DEVICE
    assert R.lib().rodent_hip_scene_create_flags(0) == gpubuild.NON_FINITE
    assert R.lib().rodent_hip_scene_motion_keys_status(0, None) < 0         # no scene is loaded then (bit 31: no deforming scene)
    with pytest.raises(gpubuild.BuildError, match="non-finite"):
        R.Renderer(scene, W, H, SPP, MAXLEN, deform=(broken, n1))
    # the entries of the other scene kinds refuse a deforming scene
    with rendering(R, parts) as r:
        import torch
        d = torch.from_numpy(v1).cuda()
        for call in (lambda: r.update_geometry(scene), lambda: r.update_geometry_device(d), lambda: r.prepare_update(),
                     lambda: r.set_transforms(d), lambda: r.set_motion_transforms(d, d), lambda: r.deform_objects(d)):
            with pytest.raises(gpubuild.BuildError, match="deforming"):
                call()
        with pytest.raises(gpubuild.BuildError, match="no instanced scene"):
            r.prepare_deform([0])
        r.render(cam, 0)                                                    # (and leave it as it was)
        assert r.film().mean() > 0.02


def test_a_non_finite_coordinate_through_set_motion_keys_is_a_status(R, parts):
    import torch
    from rodent_amd import gpubuild
    k = parts.keys
    broken = k.vertices1.copy(); broken[parts.tall[3], 1] = np.inf
    d0, d1, bad = (torch.from_numpy(a).cuda() for a in (k.vertices0, k.vertices1, broken))
    n0, n1 = (torch.from_numpy(a).cuda() for a in (k.normals0, k.normals1))
    with rendering(R, parts) as r:
        topology = r.scene_bvh()
        r.set_motion_keys(d0, bad, n0, n1, check=False)
        flags, words = r.motion_keys_status()
        assert flags == gpubuild.NON_FINITE == words[2]
        with pytest.raises(gpubuild.BuildError, match="non-finite"):
            r.set_motion_keys(d0, bad, n0, n1)
        r.set_motion_keys(d0, d1, n0, n1)                                  # a sound rebuild: the tables are the model's again
        assert r.motion_keys_status()[0] == 0
        assert_tables(r.deforming_tables(), parts, k, topology, "after a sound rebuild")
        with pytest.raises(ValueError, match="both tables of normals or neither"):
            r.set_motion_keys(d0, d1, n0, None)


def test_flat_instanced_and_moving_scenes_render_their_own_films_afterwards(R, parts, oracle, model, cam, tmp_path):
    import instanced_scene_model as IM
    import motion_scene_model as MS
    from rodent_amd import instances as I
    with rendering(R, parts, capacity=4096) as r:
        r.render(cam, 0)
        assert np.allclose(r.film(), model.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    four = {"mapping": "streaming", "trace_persistent": 0, "trace_refill": (0, 0), "sort": 0}
    objects = IM.scene_objects(GOLDEN, tmp_path)
    scene = I.concat_scenes(objects)
    hierarchy = IM.object_bvhs(scene, scene.ranges)
    transforms, ids = IM.placements()
    static = IM.frame(scene, scene.ranges, transforms, ids, hierarchy, cam, 0, SPP, MAXLEN, W, H)
    r = R.Renderer(scene, W, H, SPP, MAXLEN, instances=(scene.ranges, transforms, ids))
    assert r.options_in_effect() == four
    r.render(cam, 0)
    c = r.counters()
    assert r.trace_kernel_name() == "k_trace_instanced<true>" and r.max_path_len() == MAXLEN
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(static.counts)
    assert np.allclose(r.film(), static.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    r.close()
    t0, t1, mids = MS.placements()
    moving = MS.frame(scene, scene.ranges, t0, t1, mids, hierarchy, cam, 0, SPP, MAXLEN, W, H)
    r = R.Renderer(scene, W, H, SPP, MAXLEN, motion=(scene.ranges, t0, t1, mids))
    assert r.options_in_effect() == dict(four, max_path_len=MAXLEN, shutter=(0.0, 1.0))
    r.render(cam, 0)
    c = r.counters()
    assert r.trace_kernel_name() == "k_trace_instanced_motion<true>"
    assert (c["primary_rays"], c["shadow_rays"]) == tuple(moving.counts)
    assert np.allclose(r.film(), moving.film, rtol=FILM_RTOL, atol=FILM_ATOL)
    r.close()
    flat = R.Renderer(objects[0], W, H, SPP, MAXLEN)
    assert flat.options_in_effect() == {"mapping": "streaming", "trace_persistent": 0, "trace_refill": (0, 0), "sort": 0}
    flat.render(cam, 0)
    assert flat.trace_kernel_name().startswith("k_trace_secondary")
    want, _ = oracle.render(objects[0], cam, 0, SPP, MAXLEN, W, H)
    assert np.allclose(flat.film(), want, rtol=FILM_RTOL, atol=FILM_ATOL) and want.mean() > 0.02
    flat.close()
