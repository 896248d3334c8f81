"""tests/motion_objects_model.py, the CPU model of "deforming objects under moving instances" (include/rodent_instances.h), held to what
does not depend on it -- no GPU is needed:

* the conditions of tests/motion_objects_fixtures.py on the model alone, so that no GPU test passes vacuously;
* containment in exact rational arithmetic: every corner the kernel intersects -- v0(t), v0(t) - e1(t), v0(t) + e2(t) of the
  fp32-interpolated records -- mapped exactly by the fp32-interpolated placement lies in the instance's motion box: seeded objects at
  magnitudes 1e-3 to 1e6, the fixture, seeded placement pairs, t in {0, 1, 0.5, 2^-24, 1 - 2^-24, 33 seeded}.  The arithmetic is exact
  integer arithmetic at the fixed scale 2^-149 (every finite float32 is a multiple of it), checked against fractions.Fraction;
* with the object box taken from key 0's root alone some corner DOES lie outside: the check can fail;
* one identity instance of one object gives motion_bvh_model.trace's hits;
* equal keys everywhere with M0 == M1 gives instance_model.trace's hits over at_time(..., 0).
"""
from fractions import Fraction

import numpy as np
import pytest

import instance_model as M
import lbvh_model as L
import motion_bvh_fixtures as BX
import motion_bvh_model as B
import motion_instance_model as MI
import motion_objects_fixtures as X
import motion_objects_model as MO
from rodent_amd import formats as F

F32 = np.float32
TIMES = np.concatenate([F32([0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24]), np.random.default_rng(3).uniform(0, 1, 33).astype(F32)])
IDENTITY = F32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


@pytest.fixture(scope="module")
def block(cornell):
    return cornell.blocks[2]


@pytest.fixture(scope="module")
def scene(block):
    return X.Scene(block)


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_conditions_hold_on_the_model(oracle, block, cornell):
    figures = X.check_conditions(oracle, block, cornell)
    print(figures)
    assert len(figures["instances"]) >= 4


def test_palette_holds_the_edge_times():
    p = X.palette()
    on = B.traced(p)
    bits = lambda x: np.asarray(x, F32).view("<u4").tolist()
    for t in (-0.0, 1.0, 0.0, 0.5, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))):
        assert on[bits(p).index(bits(F32(t)))], t
    for t in (np.inf, -np.inf, np.nextafter(F32(1), F32(2)), -(2.0 ** -149)):
        assert not on[bits(p).index(bits(F32(t)))], t
    assert np.isnan(p).sum() == 1 and not on[np.isnan(p)].any()


# ---- 2. containment, exactly ------------------------------------------------------------------------------------------------------------
def exact(a):
    """float32 array -> object array of Python ints k, the value being k * 2^-149 exactly."""
    a = np.asarray(a, F32)
    assert np.isfinite(a).all()
    m, e = np.frexp(a.astype(np.float64))
    mant, shift = (m * (1 << 24)).astype(np.int64), e.astype(np.int64) - 24 + 149
    out = np.empty(a.shape, object)
    flat = out.reshape(-1)
    for k, (x, s) in enumerate(zip(mant.reshape(-1).tolist(), shift.reshape(-1).tolist())):
        assert s >= 0 or x & ((1 << -s) - 1) == 0
        flat[k] = x << s if s >= 0 else x >> -s
    return out


def test_exact_agrees_with_fractions():
    values = F32([0.0, -0.0, 1.0, -3.5, 2.0 ** -149, -(2.0 ** -140), 3.4028234664e38, 1e-3, 123456.789, 1 / 3])
    assert [Fraction(int(k), 1 << 149) for k in exact(values)] == [Fraction(float(v)) for v in values]


def corners_outside(mn, mt, m0, m1, box_rule=MO.object_box, times=TIMES, check_with_fractions=False):
    """How many corners of the object mn / mt (one object's records), at the times, mapped exactly by the fp32-interpolated placement,
    lie outside the motion box of the object box (`box_rule` of the root record) under (m0, m1)."""
    olo, ohi = box_rule(mn[:1])
    box = exact(MI.motion_box(m0, m1, olo, ohi)[0]) * (1 << 149)                        # scale 2^-298, as the images
    outside = 0
    for t in times:
        _, tris = B.at_time(mn, mt, t)
        v0, e1, e2 = exact(tris["v0"]), exact(tris["e1"]), exact(tris["e2"])
        p = np.concatenate([v0, v0 - e1, v0 + e2])
        m = exact(MI.lerp(m0, m1, t)[0]).reshape(3, 4)
        for a in range(3):
            image = p[:, 0] * m[a, 0] + p[:, 1] * m[a, 1] + p[:, 2] * m[a, 2] + m[a, 3] * (1 << 149)
            outside += int(np.array(image < box[2 * a], bool).sum()) + int(np.array(image > box[2 * a + 1], bool).sum())
            if check_with_fractions:                                                   # the same, corner 0, in fractions
                f = lambda x: Fraction(float(x))
                corner, row = [f(x) for x in tris["v0"][0]], [f(x) for x in MI.lerp(m0, m1, t)[0][4 * a: 4 * a + 4]]
                assert row[0] * corner[0] + row[1] * corner[1] + row[2] * corner[2] + row[3] == Fraction(int(image[0]), 1 << 298)
    return outside


def seeded_object(mag, seed, n=24):
    """Motion records of n scattered triangles at magnitude `mag` whose key 1 moves every vertex by up to 0.3 mag."""
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), F32)
    v[:, :3] = (rng.uniform(-mag, mag, (n, 1, 3)) + rng.uniform(-0.05 * mag, 0.05 * mag, (n, 3, 3))).reshape(-1, 3)
    ix = np.zeros((n, 4), np.int32); ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    v1 = v.copy(); v1[:, :3] += rng.uniform(-0.3 * mag, 0.3 * mag, (3 * n, 3)).astype(F32)
    nodes, tris, info = L.build(v, ix, 2)
    mn, mt, info = B.build(nodes, tris, v, v1, ix)
    assert info[2] == 0
    return mn, mt


def fixture_objects(scene):
    return [(scene.mn[o["node_offset"]:][: o["num_nodes"]], scene.mt[o["tri_offset"]:][: o["num_tris"]]) for o in scene.table]


def test_every_corner_lies_in_its_instances_motion_box(scene):
    seeded, _ = M.seeded_transforms(16, 29, 40.0, 2)
    count = 0
    for k, mag in enumerate((1e-3, 1.0, 1e3, 1e6)):                                     # seeded objects: seeded and fixture pairs
        mn, mt = seeded_object(mag, 40 + k)
        for j in range(3):
            assert corners_outside(mn, mt, seeded[4 * k + j], seeded[4 * k + j + 1], check_with_fractions=j == 0) == 0, (mag, j)
        for j in (k, X.HALF_TURN, 8):
            assert corners_outside(mn, mt, scene.t0[j], scene.t1[j]) == 0, (mag, j)
        count += 6
    objects = fixture_objects(scene)
    for j, o in enumerate(scene.obj):                                                   # the fixture: every instance, its own object
        assert corners_outside(*objects[o], scene.t0[j], scene.t1[j]) == 0, j
        count += 1
    for o, (mn, mt) in enumerate(objects):                                              # ... and every object under a seeded pair
        assert corners_outside(mn, mt, seeded[o], seeded[o + 5], times=TIMES[:12]) == 0, o
        count += 1
    assert count == 24 + 9 + 5


def test_key_0s_root_box_alone_does_not_contain_them(scene):
    """The object box must be the union over both keys: with key 0's root box the sheared cube and the soup leave their motion boxes."""
    objects = fixture_objects(scene)
    for j in (1, 2):
        assert scene.obj[j] in (X.SHEARED, X.SOUP)
        assert corners_outside(*objects[scene.obj[j]], scene.t0[j], scene.t1[j], box_rule=MO.key0_box) > 0, j
        assert corners_outside(*objects[scene.obj[j]], scene.t0[j], scene.t1[j]) == 0
    # ... and a TLAS built that way differs from the rule's
    wrong = MO.build_motion_tlas(scene.mn, scene.table, scene.descs, 1, box=MO.key0_box)
    assert wrong[0].tobytes() != scene.tlas.tobytes()


# ---- 3. anchors -------------------------------------------------------------------------------------------------------------------------
def test_one_identity_instance_gives_the_single_mesh_models_hits(oracle, scene):
    mn, mt = fixture_objects(scene)[X.SOUP]
    table = M.pack([(np.zeros(len(mn), F.NODE2), np.zeros(len(mt), F.TRI1))])[2]
    tlas, inst, info = MO.build_motion_tlas(mn, table, MI.descriptors(IDENTITY[None], IDENTITY[None], [0], [5]), 1)
    assert info[2] == 0
    rays = BX.segments(np.full(3, -0.7), np.full(3, 0.7), 1024, 5)
    times = X.times_for(len(rays))
    for any_hit in (False, True):
        hits, ids = MO.trace(oracle, tlas, inst, mn, mt, rays, times, any_hit)
        want = B.trace(oracle, mn, mt, rays, times, any_hit)
        assert hits.tobytes() == want.tobytes(), any_hit
        assert np.array_equal(ids, np.where(want["tri_id"] >= 0, 5, -1))
        assert (want["tri_id"][B.traced(times)] >= 0).mean() > 0.25
    assert (MO.peak(oracle, tlas, inst, mn, mt, rays, times) == B.peak(oracle, mn, mt, rays, times)).all()


def test_equal_keys_and_equal_placements_give_the_static_models_hits(oracle, block, cornell):
    still = X.Scene(block, freeze_objects=True, freeze_placements=True)
    nodes, tris = B.at_time(still.mn, still.mt, 0)
    assert nodes["bounds"].tobytes() == still.mn["bounds0"].tobytes() and tris.tobytes() == still.mt["key0"].tobytes()
    static = M.build_tlas(nodes, still.table, M.descriptors(still.t0, still.obj, still.ids), 1)
    assert static[2][2] == 0
    for name, rays in X.ray_sets(cornell).items():
        times = F32([0.0, 1.0])[np.arange(len(rays)) % 2]
        hits, ids = MO.trace(oracle, *still.model(), rays, times)
        want, want_ids = M.trace(oracle, static[0], static[1], nodes, tris, rays)
        assert hits.tobytes() == want.tobytes() and np.array_equal(ids, want_ids), name
