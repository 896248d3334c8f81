"""tests/motion_bvh_model.py, the CPU restatement of deforming meshes under motion (include/rodent_motion.h), on its own:

* containment in exact rational arithmetic: the three corners the kernel intersects -- v0(t), v0(t) - e1(t), v0(t) + e2(t), from the
  fp32-interpolated Tri1 -- lie in the fp32-interpolated widened leaf box, over magnitudes from 1e-3 to 1e10, steps between the keys
  from none to the size of the triangle and 39 times; with the widening set to 0 the same check finds violations;
* a parent's interpolated box contains its children's;
* the model's closest hit equals a brute force over all triangles interpolated to the ray's time (a single-leaf oracle call per time);
* the byte rules: equal keys give key0 == key1, t = 0 and t = 1 give the refitted static records as float values;
* the time rule, and the conditions of tests/motion_bvh_fixtures.py on the model alone.
"""
from fractions import Fraction

import numpy as np
import pytest

import lbvh_model as L
import motion_bvh_fixtures as X
import motion_bvh_model as MB
import refit_model as R
import trbvh_model as T
from conftest import GOLDEN
from rodent_amd import formats as F
from rodent_amd import scene as S

F32 = np.float32
TIMES = np.concatenate([F32([0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24, X.DENORMAL]),
                        np.random.default_rng(3).uniform(0.0, 1.0, 33).astype(F32)])


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


@pytest.fixture(scope="module")
def fixture_shapes(cornell_scene, cornell):
    """[(shape, topology nodes, topology tris, motion nodes, motion tris)] over lbvh_model's max_leaf 2 tree of key 0."""
    out = []
    for sh in X.shapes(cornell_scene, cornell):
        nodes, tris, info = L.build(sh.v0, sh.ix, 2)
        assert info[2] == 0
        out.append((sh, nodes, tris, *sh.records(nodes, tris)))
    return out


# ---- containment ------------------------------------------------------------------------------------------------------------------------
def triangle_pairs(seed, count=60):
    """(v0 (m, 9), v1 (m, 9)) float32: m triangle pairs, one row = 3 corners x 3 axes, over magnitudes 1e-3 ... 1e10, triangle sizes
    from 1e-4 of the magnitude to the magnitude, and steps between the keys of none, 1e-6 of the size, and the size."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for mag in (1e-3, 1.0, 37.0, 1e4, 1e10):
        for size in (1e-4, 1e-2, 1.0):
            for step in (0.0, 1e-6, 1.0):
                centre = rng.uniform(-mag, mag, (count, 1, 3))
                k0 = centre + rng.uniform(-size * mag, size * mag, (count, 3, 3))
                k1 = k0 + step * rng.uniform(-size * mag, size * mag, (count, 3, 3))
                a.append(k0.reshape(count, 9)); b.append(k1.reshape(count, 9))
    return np.concatenate(a).astype(F32), np.concatenate(b).astype(F32)


def leaf_records(k0, k1, widen):
    """One single-triangle leaf per pair through the model: (mn, mt) where node i holds pair i in slot 0."""
    m = len(k0)
    v0 = np.zeros((3 * m, 4), F32); v0[:, :3] = k0.reshape(-1, 3)
    v1 = np.zeros((3 * m, 4), F32); v1[:, :3] = k1.reshape(-1, 3)
    ix = np.zeros((m, 4), np.int32); ix[:, :3] = np.arange(3 * m).reshape(m, 3)
    # a topology of m root-like nodes, each with its own one-triangle leaf in slot 0: the refit model needs no more than that
    nodes, tris = np.zeros(m, F.NODE2), np.zeros(m, F.TRI1)
    nodes["child"][:, 0] = ~np.arange(m)
    nodes["bounds"][:, 6::2], nodes["bounds"][:, 7::2] = np.inf, -np.inf
    tris["prim_id"] = np.arange(m) | np.int32(-2 ** 31)
    mn, mt, info = MB.build(nodes, tris, v0, v1, ix, widen)
    assert info[2] == 0 and info[1] == 2 * m
    return mn, mt


def corners_outside(mn, mt, times, stride=1):
    """(checks, violations): per pair, time, corner and axis, whether the kernel's corner -- exact: Fractions of the fp32-interpolated
    record -- lies outside the fp32-interpolated box of slot 0."""
    checks = bad = 0
    for t in times:
        nodes, tris = MB.at_time(mn, mt, t)
        box = nodes["bounds"][::stride, :6]
        v0, e1, e2 = tris["v0"][::stride], tris["e1"][::stride], tris["e2"][::stride]
        for i in range(len(box)):
            for a in range(3):
                lo, hi = Fraction(float(box[i, 2 * a])), Fraction(float(box[i, 2 * a + 1]))
                p = Fraction(float(v0[i, a]))
                for c in (p, p - Fraction(float(e1[i, a])), p + Fraction(float(e2[i, a]))):
                    checks += 1
                    bad += not lo <= c <= hi
    return checks, bad


def test_kernel_corners_lie_in_the_interpolated_widened_box():
    k0, k1 = triangle_pairs(1, 12)
    mn, mt = leaf_records(k0, k1, MB.WIDEN)
    checks, bad = corners_outside(mn, mt, TIMES)
    print(f"{checks} corner / axis checks at 2^-19: {bad} outside")
    assert checks > 150_000 and bad == 0
    # not vacuous: without the widening the same check fails
    mn0, mt0 = leaf_records(k0, k1, 0.0)
    checks0, bad0 = corners_outside(mn0, mt0, TIMES[[0, 1, 2, 3, 4, 5, 6, 7]])
    print(f"{checks0} checks with no widening: {bad0} outside ({100.0 * bad0 / checks0:.1f} %)")
    assert bad0 > checks0 // 100


def test_a_parents_interpolated_box_contains_its_childrens(fixture_shapes):
    rng = np.random.default_rng(8)
    cases = [(sh.name, mn) for sh, _, _, mn, _ in fixture_shapes]
    # ... and trees over scattered triangles at magnitudes from 1e-3 to 1e10 with steps as large as the mesh
    for mag in (1e-3, 1.0, 1e4, 1e10):
        v = np.zeros((3 * 300, 4), F32)
        v[:, :3] = (rng.uniform(-mag, mag, (300, 1, 3)) + rng.uniform(-0.05 * mag, 0.05 * mag, (300, 3, 3))).reshape(-1, 3)
        ix = np.zeros((300, 4), np.int32); ix[:, :3] = np.arange(900).reshape(300, 3)
        v1 = v.copy(); v1[:, :3] += rng.uniform(-0.3 * mag, 0.3 * mag, (900, 3)).astype(F32)
        nodes, tris, _ = T.build(v, ix, 2, passes=1)
        cases.append((f"scattered{mag:g}", MB.build(nodes, tris, v, v1, ix)[0]))
    for name, mn in cases:
        child = mn["child"]
        up, slot = np.nonzero(child > 0)
        below = child[up, slot] - 1
        for t in TIMES:
            b = MB.at_time(mn, np.zeros(0, F.MOTION_TRI1), t)[0]["bounds"]
            outer = b[up[:, None], 6 * slot[:, None] + np.arange(6)]
            for k in range(2):
                inner, used = b[below, 6 * k: 6 * k + 6], child[below, k] != 0
                ok = (outer[:, 0::2] <= inner[:, 0::2]).all(1) & (outer[:, 1::2] >= inner[:, 1::2]).all(1)
                assert ok[used].all(), (name, float(t))


# ---- the model against a brute force ----------------------------------------------------------------------------------------------------
def single_leaf(tris):
    """The one-node hierarchy with every record of `tris` in one leaf."""
    nodes, t = np.zeros(1, F.NODE2), tris.copy()
    nodes["bounds"][0, :6] = [-np.inf, np.inf] * 3
    nodes["bounds"][0, 6:] = [np.inf, -np.inf] * 3
    nodes["child"][0] = [~0, 0]
    t["prim_id"] &= 0x7FFFFFFF
    t["prim_id"][-1] |= np.int32(-2 ** 31)
    return nodes, t


def test_closest_hit_equals_the_brute_force_at_the_rays_time(oracle, fixture_shapes):
    for sh, _, _, mn, mt in fixture_shapes:
        for name, rays in sh.rays.items():
            times = X.times_for(len(rays))
            got = MB.trace(oracle, mn, mt, rays, times)
            assert MB.peak(oracle, mn, mt, rays, times).max() <= 63
            for t, sel in MB.time_groups(times):
                if not MB.traced(t):
                    continue
                brute = oracle.traverse(2, *single_leaf(MB.at_time(mn, mt, t)[1]), rays[sel])[0]
                assert np.array_equal(got["t"][sel], brute["t"]), (sh.name, name, float(t))
                assert np.array_equal(got["tri_id"][sel] >= 0, brute["tri_id"] >= 0), (sh.name, name, float(t))


# ---- byte rules -------------------------------------------------------------------------------------------------------------------------
def test_equal_keys_give_equal_records(fixture_shapes):
    for sh, nodes, tris, _, _ in fixture_shapes:
        mn, mt, info = MB.build(nodes, tris, sh.v0, sh.v0, sh.ix)
        assert info.tolist() == [len(nodes), len(nodes) + len(tris), 0, len(nodes)]
        assert mn["bounds0"].tobytes() == mn["bounds1"].tobytes()
        for name in MB.GEOMETRY:
            assert mt["key0"][name].tobytes() == mt["key1"][name].tobytes()
        assert not mt["key1"]["pad"].any() and not mt["key1"]["geom_id"].any() and not mt["key1"]["prim_id"].any()
        assert np.array_equal(mt["key0"]["prim_id"], tris["prim_id"]) and np.array_equal(mt["key0"]["geom_id"], tris["geom_id"])
        # the widening: every taken slot's stored box contains the refitted one, an empty slot keeps its bytes
        refitted = R.refit(nodes, tris, sh.v0, sh.ix)[0]["bounds"]
        taken = np.repeat(nodes["child"] != 0, 6, axis=1)
        assert (mn["bounds0"][:, 0::2] <= refitted[:, 0::2])[taken[:, 0::2]].all()
        assert (mn["bounds0"][:, 1::2] >= refitted[:, 1::2])[taken[:, 1::2]].all()
        assert mn["bounds0"][~taken].tobytes() == refitted[~taken].tobytes()


def test_times_zero_and_one_give_the_static_records_as_values(fixture_shapes):
    for sh, nodes, tris, mn, mt in fixture_shapes:
        for t, v in ((0.0, sh.v0), (1.0, sh.v1), (-0.0, sh.v0)):
            static = R.refit(nodes, tris, v, sh.ix)[1]
            lerped = MB.at_time(mn, mt, F32(t))[1]
            for name in MB.GEOMETRY:
                assert np.array_equal(lerped[name], static[name]), (sh.name, t, name)      # as float values: -0 == +0
            for name in MB.WORDS:
                assert np.array_equal(lerped[name], static[name]), (sh.name, t, name)
            key = mn["bounds0"] if v is sh.v0 else mn["bounds1"]
            taken = np.repeat(mn["child"] != 0, 6, axis=1)
            assert np.array_equal(MB.at_time(mn, mt, F32(t))[0]["bounds"][taken], key[taken])


def test_fuse_flags_a_second_topology(fixture_shapes):
    sh, nodes, tris, _, _ = fixture_shapes[1]
    n0, t0, _ = R.refit(nodes, tris, sh.v0, sh.ix)
    n1, t1, _ = R.refit(nodes, tris, sh.v1, sh.ix)
    assert MB.fuse(n0, t0, n1, t1)[2].tolist() == [0, len(n0) + len(t0), 0, 0]
    swapped = n1.copy(); swapped["child"][3] = swapped["child"][3][::-1].copy()
    mn, _, info = MB.fuse(n0, t0, swapped, t1)
    assert info[2] == MB.BAD_TOPOLOGY and np.array_equal(mn["child"], n0["child"])
    other = t1.copy(); other["geom_id"][5] += 1
    mt, info = MB.fuse(n0, t0, n1, other)[1:]
    assert info[2] == MB.BAD_TOPOLOGY and np.array_equal(mt["key0"]["geom_id"], t0["geom_id"]) and not mt["key1"]["geom_id"].any()


# ---- the time rule, and the fixtures' conditions ----------------------------------------------------------------------------------------
def test_the_time_rule(oracle, fixture_shapes):
    refused = F32([np.nan, np.inf, -np.inf, -(2.0 ** -149), np.nextafter(F32(1), F32(2)), -0.25, 1.5])
    assert not MB.traced(refused).any() and MB.traced(F32([-0.0, 1.0, 0.0, X.DENORMAL])).all()
    assert np.array_equal(refused.view("<u4"), X.REFUSED.view("<u4"))
    sh, _, _, mn, mt = fixture_shapes[0]
    rays = sh.rays["primary"][:256]
    for t in refused:
        hits = MB.trace(oracle, mn, mt, rays, np.full(len(rays), t, F32))
        assert (hits["tri_id"] == -1).all() and hits["t"].tobytes() == rays["tmax"].tobytes()
        assert not hits["u"].any() and not hits["v"].any()
    for t in F32([-0.0, 1.0]):
        assert (MB.trace(oracle, mn, mt, rays, np.full(len(rays), t, F32))["tri_id"] >= 0).mean() > 0.5


def test_the_fixtures_meet_their_conditions(oracle, fixture_shapes):
    for sh, _, _, mn, mt in fixture_shapes:
        for name, (share, moved, flipped) in X.check_conditions(oracle, sh, mn, mt).items():
            print(f"{sh.name} {name}: {100 * share:.1f} % of the traced rays hit, {100 * moved:.1f} % of the hits at t = 0.5 differ from "
                  f"both keys, {flipped} rays hit at one key only")
