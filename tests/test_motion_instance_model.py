"""tests/motion_instance_model.py held to the rules of "moving instances" (include/rodent_instances.h) on the CPU, and the fixture of
tests/test_gpu_motion_instances.py shown not to be vacuous.

* lerp returns the endpoints at t = 0 and t = 1, the inverse at t = 0 is instance_model.invert(M0);
* the motion box contains, in exact rational arithmetic, the image of all 8 object-box corners under the fp32-interpolated matrix;
* the model's closest hits equal a float64 brute force over every (instance, triangle) placed at the ray's own time;
* the fixture: records depend on the times, hits and misses in every time group, rays that meet a skipped instance;
* all times 0 gives the static model's records over M0;
* every host-side refusal of the three build entry points, in the stated order (dev = -1: no GPU is touched).
"""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import instance_edge_fixtures as E
import instance_model as M
import motion_instance_fixtures as X
import motion_instance_model as MM

F32 = np.float32
TIMES = np.concatenate([F32([0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-40]),
                        np.random.default_rng(33).uniform(0.0, 1.0, 33).astype(F32)])


@pytest.fixture(scope="module")
def block(cornell):
    return cornell.blocks[2]


@pytest.fixture(scope="module")
def scene(block):
    return X.Scene(block)


@pytest.fixture(scope="module")
def traced(oracle, scene, cornell):
    """{name: (rays, times, model hits, model instance ids)} of the fixture's two ray sets, closest hit."""
    return {name: (rays, times, *MM.trace(oracle, *scene.model(), rays, times)) for name, (rays, times) in X.ray_sets(cornell).items()}


def bits(a):
    return np.ascontiguousarray(a, F32).view("<u4")


# ---- 1. endpoints -------------------------------------------------------------------------------------------------------------------------
def matrix_pool():
    a, _ = M.seeded_transforms(40, 3, 40.0, 2)
    return np.concatenate([a, np.array([m for _, m, _ in E.edge_matrices()])])


def test_lerp_returns_the_endpoints_and_the_static_inverse():
    pool = matrix_pool()
    other = np.roll(pool, 7, axis=0)
    # Bit for bit, but for the one case two products and a sum cannot keep (the header's note; the edge set holds such entries): an
    # entry -0 beside a positive partner comes out as 1 * -0 + 0 * m1 = -0 + +0 = +0, equal as a value.  Every matrix without a -0
    # entry keeps all its bits, and its inverse all of its own; with one, the inverse differs at most in the sign of a zero.
    minus_zero = lambda a: np.signbit(a) & (a == 0)
    flips = 0
    for a, t in ((pool, 0.0), (other, 1.0)):
        got = MM.lerp(pool, other, t)
        flipped = bits(got) != bits(a)
        assert np.array_equal(got, a) and (flipped <= minus_zero(a)).all()
        flips += int(flipped.sum())
    plain = ~minus_zero(pool).any(1)
    assert flips > 0 and plain.sum() >= 50
    w, bad = M.invert(pool)
    w0, bad0 = M.invert(MM.lerp(pool, other, 0.0))
    assert not bad.any() and not bad0.any() and np.array_equal(bits(w)[plain], bits(w0)[plain])
    assert np.array_equal(w, w0) and ((bits(w) != bits(w0)) <= (w == 0)).all()
    # the case made by hand
    m0, m1 = pool[0].copy(), pool[1].copy()
    m0[3], m1[3] = -0.0, 2.0
    got = MM.lerp(m0, m1, 0.0)[0]
    assert np.array_equal(got, m0) and bits(got)[3] == 0 and np.array_equal(np.delete(bits(got), 3), np.delete(bits(m0), 3))
    assert np.array_equal(M.invert(got)[0], M.invert(m0)[0])
    # a time per matrix, and a NaN time: every entry NaN, every instance skipped
    per = MM.lerp(pool, other, np.where(np.arange(len(pool)) % 2, F32(1), F32(0)))
    assert np.array_equal(per, np.where((np.arange(len(pool)) % 2)[:, None], other, pool))
    assert np.isnan(MM.lerp(pool, other, np.nan)).all() and M.invert(MM.lerp(pool, other, np.nan))[1].all()
    # the half turn: singular at 0.5 exactly, sound on either side
    t0, t1, _, _ = X.layout()
    h = X.HALF_TURN
    assert M.invert(MM.lerp(t0[h], t1[h], 0.5))[1][0]
    assert not any(M.invert(MM.lerp(t0[h], t1[h], t))[1][0] for t in (0.0, 1.0, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))))


# ---- 2. containment -----------------------------------------------------------------------------------------------------------------------
def frac(a):
    return [Fraction(float(x)) for x in np.asarray(a, F32).reshape(-1)]


def contained(m0, m1, lo, hi, times=TIMES):
    """Whether the motion box contains the exact image of the 8 corners of (lo, hi) under lerp(m0, m1, t) for every t of `times`."""
    box = frac(MM.motion_box(m0, m1, lo[None], hi[None])[0])
    corners = [[frac(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)]
    for t in times:
        m = frac(MM.lerp(m0, m1, t))
        for a in range(3):
            images = [m[4 * a] * p[0] + m[4 * a + 1] * p[1] + m[4 * a + 2] * p[2] + m[4 * a + 3] for p in corners]
            if not (box[2 * a] <= min(images) and max(images) <= box[2 * a + 1]):
                return False
    return True


def test_motion_boxes_contain_every_placement_exactly(block):
    nodes, _, table = M.pack([block, M.flat_object()])
    boxes = [M.object_box(nodes[offset]) for offset in table["node_offset"]]          # the Cornell block's and the flat object's
    rng = np.random.default_rng(5)
    seeded, _ = M.seeded_transforms(48, 17, 40.0, 2)
    count = 0
    for k in range(24):                                                               # seeded pairs, seeded object boxes
        a, b = rng.uniform(-3, 3, 3).astype(F32), rng.uniform(-3, 3, 3).astype(F32)
        assert contained(seeded[2 * k], seeded[2 * k + 1], np.fmin(a, b), np.fmax(a, b)), k
    edge = E.edge_matrices()
    for (n0, m0, o0), (n1, m1, _) in itertools.product(edge, edge):                   # the edge matrices with each other, same ones too
        assert contained(m0, m1, *boxes[o0], TIMES[:6]), (n0, n1)
        count += 1
    for (n0, m0, o0), (n1, m1, _) in zip(edge, edge[5:] + edge[:5]):                  # ... and a cycle of them over all 39 times
        assert contained(m0, m1, *boxes[o0]), (n0, n1)
    t0, t1, obj, _ = X.layout()                                                       # the GPU fixture, its half-turn pair among them
    cube_box = M.object_box(X.cube()[0][0])
    for k in range(len(obj)):
        assert contained(t0[k], t1[k], *(boxes[0] if obj[k] == 0 else cube_box)), k
    assert count == len(edge) ** 2


def test_underflowing_products_stay_outside_the_domain():
    """The static rule's pinned case (entries and coordinates ~ 1e-22, no translation) under motion: the endpoint boxes miss corners
    already, the motion box's second widening is as relative as the first.  The same draws at an ordinary scale are contained."""
    for scale, expect in ((1e-22, False), (1.0, True)):
        rng = np.random.default_rng(22)
        inside = 0
        for _ in range(20):
            m0, m1 = ((rng.uniform(-1, 1, 12) * scale).astype(F32) for _ in range(2))
            if not expect:
                m0[3::4] = m1[3::4] = 0
            a, b = ((rng.uniform(-1, 1, 3) * scale).astype(F32) for _ in range(2))
            inside += contained(m0, m1, np.fmin(a, b), np.fmax(a, b), TIMES[:12])
        print(f"scale {scale}: {inside} of 20 motion boxes contain every image")
        assert inside == 20 if expect else inside <= 5


# ---- 3. the model against float64 ---------------------------------------------------------------------------------------------------------
def test_model_against_float64_moeller_trumbore(scene, traced):
    """Compared: rays with a time in [0, 1] (outside it the motion box promises nothing: the walk may pass an instance by, and the
    kernel does so with it), at most 2 % of them left out as ambiguous (GAP and MARGIN of the fixtures).  t: within 1e-4 * max(t, 1) --
    the object ray comes through an fp32 inverse whose entries reach 1 / 0.022 ~ 45 for the half turn at the palette's 0.4725, on
    origins up to ~5: some 10 roundings of 2^-24 * 45 * 5 each stay below 1e-4 in object units of >= 0.2 world units."""
    for name, (rays, times, hits, ids) in traced.items():
        ok = (times >= 0) & (times <= 1)
        b_inst, b_prim, b_t, left_out = X.brute_force(scene, rays, times)
        share = left_out[ok].mean()
        print(f"{name}: {ok.sum()} rays compared, {share:.4f} left out, hit share {np.isfinite(b_t[ok]).mean():.3f}")
        assert share <= 0.02
        keep = ok & ~left_out
        hit = hits["tri_id"] >= 0
        assert np.array_equal(hit[keep], np.isfinite(b_t[keep]))
        k = keep & hit
        assert np.array_equal(ids[k], b_inst[k]) and np.array_equal(hits["tri_id"][k], b_prim[k])
        assert (np.abs(hits["t"][k] - b_t[k]) <= 1e-4 * np.maximum(b_t[k], 1.0)).all()
        assert (ids[keep & ~hit] == -1).all() and np.array_equal(bits(hits["t"][~hit]), bits(rays["tmax"][~hit]))


# ---- 4. the fixture is not vacuous --------------------------------------------------------------------------------------------------------
class CountingSkips(MM._Skipping):
    met = 0

    def traverse(self, width, nodes, tris, ray, any_hit=False):
        CountingSkips.met += len(nodes) == 0
        return super().traverse(width, nodes, tris, ray, any_hit)


def test_fixture_depends_on_the_times(oracle, scene, traced, monkeypatch):
    for name, (rays, times, hits, ids) in traced.items():
        h0, i0 = MM.trace(oracle, *scene.model(), rays, np.zeros(len(rays), F32))
        differ = (hits.view("<u4").reshape(-1, 4) != h0.view("<u4").reshape(-1, 4)).any(1) | (ids != i0)
        print(f"{name}: {differ.mean():.3f} of the rays have another record at their own time than at 0")
        assert differ.mean() >= 0.25
        groups = MM.time_groups(times)
        assert len(groups) == 16
        for t, sel in groups:
            got = hits["tri_id"][sel] >= 0
            assert (not got.any()) if np.isnan(t) else (got.any() and not got.all()), (name, t)     # a NaN time: every instance skipped
        assert len(set(ids[ids >= 0])) == 9
    # rays that meet a skipped instance: the half turn at 0.5, everything at NaN
    monkeypatch.setattr(MM, "_Skipping", CountingSkips)
    rays, times, hits, ids = traced["primary"]
    for t in (F32(0.5), F32(np.nan)):
        sel = np.flatnonzero(bits(times) == bits([t])[0])
        CountingSkips.met = 0
        again = MM.trace(oracle, *scene.model(), rays[sel], times[sel])
        print(f"t = {t}: {CountingSkips.met} skipped instances met by {len(sel)} rays")
        assert CountingSkips.met >= 10 and again[0].tobytes() == hits[sel].tobytes()
    sel = np.flatnonzero((times > 0) & (times < 0.4))                     # a sound time: nothing is skipped
    CountingSkips.met = 0
    MM.trace(oracle, *scene.model(), rays[sel], times[sel])
    assert CountingSkips.met == 0


def test_half_turn_rays_see_the_cube_at_0_and_what_lies_behind_it_at_half(oracle, scene):
    rays = X.half_turn_rays(scene)
    own = int(scene.ids[X.HALF_TURN])
    h0, i0 = MM.trace(oracle, *scene.model(), rays, np.zeros(len(rays), F32))
    h5, i5 = MM.trace(oracle, *scene.model(), rays, np.full(len(rays), 0.5, F32))
    assert (i0 == own).mean() > 0.9
    assert (i5 != own).all() and (i5[i0 == own] >= 0).mean() > 0.9 and np.isfinite(h5["t"]).all()
    assert (h5["t"][(i0 == own) & (i5 >= 0)] > h0["t"][(i0 == own) & (i5 >= 0)]).all()


# ---- all times 0: the static model over M0 ------------------------------------------------------------------------------------------------
def test_all_times_zero_is_the_static_model_over_m0(oracle, scene, cornell):
    """The static TLAS over M0 is another tree than the motion TLAS (other boxes), so the records agree because no two instances
    coincide: no hit is decided by the order in which instances are met."""
    static = M.build_tlas(scene.nodes, scene.table, M.descriptors(scene.t0, scene.obj, scene.ids), 1)
    for name, (rays, _) in X.ray_sets(cornell).items():
        for any_hit in (False,):
            a = MM.trace(oracle, *scene.model(), rays, np.zeros(len(rays), F32), any_hit)
            b = M.trace(oracle, static[0], static[1], scene.nodes, scene.tris, rays, any_hit)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), name


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
NUM_INSTANCES, MAX_LEAF, NUM_OBJECTS, NULL, DEVICE = -14, -2, -15, -4, -5
POINTERS = ("nodes", "objects", "descs", "tlas_nodes", "instances", "scratch", "info_dev")
GOOD = dict(nodes=0x1000, objects=0x2000, num_objects=2, descs=0x3000, num_instances=9, max_leaf=1, tlas_nodes=0x4000,
            instances=0x5000, scratch=0x6000, info_dev=0x7000)
ARGS = ("nodes", "objects", "num_objects", "descs", "num_instances", "max_leaf", "tlas_nodes", "instances", "scratch", "info_dev")
CLASSES = {"num_instances": [("num_instances", 0), ("num_instances", -1), ("num_instances", (1 << 22) + 1)],
           "max_leaf": [("max_leaf", 0), ("max_leaf", 9)],
           "num_objects": [("num_objects", 0), ("num_objects", -3)],
           **{f"null_{p}": [(p, None)] for p in POINTERS}}
ORDER = {"num_instances": NUM_INSTANCES, "max_leaf": MAX_LEAF, "num_objects": NUM_OBJECTS, **{f"null_{p}": NULL for p in POINTERS}}


@pytest.fixture(scope="module")
def l(native_build):
    from rodent_amd import abi
    return abi.lib()


def test_refusals_of_the_motion_build_entries_in_their_order(l):
    call = lambda bad: l.rodent_hip_build_motion_tlas(-1, *[{**GOOD, **bad}[k] for k in ARGS], None)
    assert call({}) == DEVICE                                            # nothing wrong but the device
    rank, count = list(ORDER), 0
    singles = [((c,), dict([kv])) for c, bad in CLASSES.items() for kv in bad]
    doubles = [((c0, c1), dict([b0[0], b1[0]])) for (c0, b0), (c1, b1) in itertools.combinations(CLASSES.items(), 2)]
    for classes, bad in singles + doubles:
        assert call(bad) == ORDER[min(classes, key=rank.index)], bad
        count += 1
    assert count >= 2 * len(ORDER)
    # the sync form: the instance count, max_leaf, the device -- then the asynchronous entry's own checks, which a bad device hides
    sync = lambda **bad: l.rodent_hip_build_motion_tlas_sync(-1, *[{**GOOD, **bad}[k] for k in ARGS[:8]], None)
    assert sync() == DEVICE and sync(num_instances=0) == NUM_INSTANCES and sync(num_instances=(1 << 22) + 1) == NUM_INSTANCES
    assert sync(num_instances=0, max_leaf=0) == NUM_INSTANCES and sync(max_leaf=9) == MAX_LEAF
    assert sync(num_objects=0) == DEVICE and sync(nodes=None) == DEVICE
    # the scratch size: -1 outside [1, 2^22], never less than the static build's (a record of twice the size is staged)
    assert l.rodent_hip_motion_tlas_scratch_bytes(0) == -1 and l.rodent_hip_motion_tlas_scratch_bytes((1 << 22) + 1) == -1
    for n in (1, 9, 1000, 1 << 22):
        assert l.rodent_hip_motion_tlas_scratch_bytes(n) >= l.rodent_hip_tlas_scratch_bytes(n) + 64 * n - 256      # (256-byte carving)
