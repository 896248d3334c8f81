"""The CPU model of moving instances in the renderer (tests/motion_scene_model.py) against the rules of include/rodent_render.h: the
shutter rule over every time a path can draw, the depth word, the model's frame beside the static instanced model's at M0, and that
the frame and the crafted trace set contain what the GPU tests rely on."""
import numpy as np
import pytest

import instanced_scene_model as IM
import motion_instance_model as MM
import motion_scene_model as MS
from conftest import GOLDEN
from rodent_amd import instances as I, render as R, scene as S

F32 = np.float32
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = MS.W, MS.H, MS.SPP, MS.MAXLEN
ALL_UBITS = np.arange(1 << 23, dtype=np.int32)


@pytest.fixture(scope="module")
def parts(oracle, tmp_path_factory):
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("motion_model"))
    scene = I.concat_scenes(objects)
    return scene, scene.ranges, IM.object_bvhs(scene, scene.ranges)


@pytest.fixture(scope="module")
def cam():
    return S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)


@pytest.fixture(scope="module")
def model(parts, cam):
    scene, ranges, hierarchy = parts
    t0, t1, ids = MS.placements()
    return MS.frame(scene, ranges, t0, t1, ids, hierarchy, cam, 0, SPP, MAXLEN, W, H)


# ---- the shutter rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(0.0, 1.0), (0.25, 0.75), (1 / 3, 1 / 3), (0.0, 2.0 ** -24), (1 - 2.0 ** -24, 1.0)])
def test_every_time_lies_in_the_shutter(pair):
    o, c = F32(pair[0]), F32(pair[1])
    t = MS.shutter_time(ALL_UBITS, o, c)
    assert t.dtype == F32 and (t >= o).all() and (t <= c).all()
    if pair == (0.0, 1.0):                                                 # t == u bit for bit
        u = (np.uint32(127 << 23) | ALL_UBITS.astype(np.uint32)).view(F32) - F32(1)           # randf's expression
        assert np.array_equal(t.view(np.uint32), u.view(np.uint32))


def test_seeded_shutters_keep_their_times_inside():
    rng = np.random.default_rng(11)
    for _ in range(64):
        o, c = np.sort(rng.random(2).astype(F32))
        t = MS.shutter_time(rng.integers(0, 1 << 23, 4096), o, c)
        assert (t >= o).all() and (t <= c).all() and 0 <= o <= c <= 1


# ---- the depth word -----------------------------------------------------------------------------------------------------------------------
def test_depth_words_round_trip():
    depth, ubits = np.meshgrid([0, 254, 255], [0, 1 << 22, (1 << 23) - 1], indexing="ij")
    words = R.pack_depth_time(depth, ubits)
    assert words.dtype == np.int32 and (words >= 0).all()                  # bit 31 is never set
    assert np.array_equal(words, MS.pack(depth, ubits))
    d, u = R.unpack_depth_time(words)
    assert np.array_equal(d, depth) and np.array_equal(u, ubits)
    assert (R.MOTION_DEPTH_BITS, R.MOTION_DEPTH_MASK) == (MS.DEPTH_BITS, MS.DEPTH_MASK) == (8, 0xFF)
    for bad in ((256, 0), (-1, 0), (0, 1 << 23), (0, -1)):
        with pytest.raises(ValueError):
            R.pack_depth_time(*bad)


def test_the_third_draw_is_randf():
    rnd = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x811C9DC5], np.uint32)
    after, ubits = MS.third_draw(rnd)
    want = []
    for x in rnd.tolist():                                                 # random.impala:22-30 in Python integers
        x = x or 1
        x ^= (x << 13) & 0xFFFFFFFF; x ^= x >> 17; x ^= (x << 5) & 0xFFFFFFFF
        want.append(x)
    assert after.tolist() == want and ubits.tolist() == [x & 0x7FFFFF for x in want]


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------
def test_shutter_0_0_is_the_static_instanced_model_at_m0(parts, cam, monkeypatch):
    """With every time 0 the placements are M0 (1 * m0 + 0 * m1; a -0 entry becomes +0, which changes no product's value), so the frame
    is the static instanced model's at M0 -- given the same random states: that model draws no shutter sample, so its emit_samples is
    wrapped to hand it the state behind the third draw."""
    scene, ranges, hierarchy = parts
    t0, t1, ids = MS.placements()                                           # (no coincident pair among these placements)
    moving = MS.frame(scene, ranges, t0, t1, ids, hierarchy, cam, 0, SPP, MAXLEN, W, H, shutter=(0.0, 0.0))
    emit = IM.O.emit_samples
    monkeypatch.setattr(IM.O, "emit_samples", lambda *a: (lambda rnd, d: (MS.third_draw(rnd)[0], d))(*emit(*a)))
    static = IM.frame(scene, ranges, t0, ids, hierarchy, cam, 0, SPP, MAXLEN, W, H)
    assert moving.counts == static.counts and moving.counts[0] > W * H * SPP and moving.counts[1] > 500
    assert np.allclose(moving.film, static.film, rtol=FILM_RTOL, atol=FILM_ATOL) and static.film.mean() > 0.02


def test_the_frame_and_the_crafted_rays_contain_what_the_gpu_tests_rely_on(parts, oracle, model):
    scene, ranges, (nodes, tris, table) = parts
    t0, t1, ids = MS.placements()
    rays, _, hits, own, ubits = model.primary[0]
    assert len(rays) == W * H * SPP and np.array_equal(ubits, model.ubits)
    _, at0 = MM.trace(oracle, model.tlas, model.instances, nodes, tris, rays, np.zeros(len(rays), F32))
    mover, mover0 = np.isin(own, MS.MOVERS), np.isin(at0, MS.MOVERS)
    assert (mover & (at0 != own)).sum() >= 1, "a ray that hits a mover but would miss it at M0"
    assert (mover0 & (at0 != own)).sum() >= 1, "a ray that misses a mover but would hit it at M0"
    assert np.isin(own, (MS.BOX, MS.QUAD_A, MS.QUAD_B)).sum() >= 1, "a ray that hits a static part"
    assert set(np.unique(own[own >= 0])) >= {MS.BOX, MS.QUAD_A, MS.SLIDER, MS.TUMBLER, MS.MIRRORED, MS.HALF_TURN}
    crafted, cu = MS.crafted_rays(t0)
    n = len(crafted) // 4
    for shutter in ((0.0, 1.0), (0.25, 0.75)):
        times = MS.shutter_time(cu, *shutter)
        assert (times[n:2 * n] == F32(0.5)).all()
        _, ci = MM.trace(oracle, model.tlas, model.instances, nodes, tris, crafted, times)
        at_start, at_half = ci[:n], ci[n:2 * n]
        # the same ray: the half-turn cube hit at one time, skipped (the box behind it answers) at t = 0.5
        assert ((at_start == MS.HALF_TURN) & (at_half == MS.BOX)).sum() >= 4 and (at_half != MS.HALF_TURN).all()
        assert set(ci.tolist()) >= {-1, MS.BOX, MS.SLIDER, MS.TUMBLER, MS.MIRRORED, MS.HALF_TURN}
    _, skipped = MM.placed(model.instances, F32(0.5), len(nodes))
    assert skipped.sum() == 1 and (model.instances["instance_id"][skipped] & 0x7FFFFFFF) == MS.HALF_TURN


def test_world_lights_are_the_static_ones_at_m0(parts):
    scene, ranges, _ = parts
    t0, t1, ids = MS.placements()
    assert not MS.moving_light(ranges, t0, t1, ids) and t0[1:3].tobytes() == t1[1:3].tobytes()
    assert MS.world_lights(scene.lights, ranges, t0, ids).tobytes() == IM.world_lights(scene.lights, ranges, t0, ids).tobytes()
    moved = t1.copy(); moved[MS.QUAD_B, 3] += F32(0.25)
    assert MS.moving_light(ranges, t0, moved, ids)
