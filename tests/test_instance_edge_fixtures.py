"""tests/instance_edge_fixtures.py is not vacuous (CPU only): every ray class holds hits and misses by the model alone, an independent
float64 Moeller-Trumbore over the transformed triangles agrees with the model on the ordinary rays, each named perturbation of the model
shows in the expectations, the widened world boxes contain the exact corner images (exact rational arithmetic) wherever no product
underflows and demonstrably not below that, and the flag boundary and the stack layouts land where they were meant to.

Two properties of these tests that follow from the arithmetic:
* class e (tmax = the model's t and its neighbours) cannot be judged hit / miss by float64 arithmetic: the decision lies one ulp of
  float32 from t.  Its rays go through the independent check with tmax = FLT_MAX (the rays themselves, their t to rtol 1e-4).
* dropping copysign in instance_model.make_ray (the TLAS's world ray; the object's own is the oracle's C) cannot change a hit RECORD:
  negating inv_dir on an axis maps that axis's slab interval [near, far] to [-far, -near]; a ray that hits an instance is inside the
  instance's widened box on an axis it does not move along, where both intervals straddle 0 and entry and exit are decided by the other
  axes.  What it changes is which instances a ray ENTERS when it runs a few denormal steps beside a box that is flat and not widened, so
  that is what the test asserts, together with the records of classes b and d staying as they are.
"""
from fractions import Fraction

import numpy as np
import pytest

import instance_edge_fixtures as E
import instance_model as M
from conftest import ambiguous_mask
from rodent_amd import formats as F

AMBIGUOUS_CAP = 0.05
TINY = np.float32(1e-8)


@pytest.fixture(scope="module")
def block(cornell):
    return cornell.blocks[2]


# ---- class counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top,cls", E.CASES)
def test_every_class_hits_and_misses(oracle, block, top, cls):
    hits, ids = E.expect(oracle, block, top, 1, cls, False)
    hit = hits["tri_id"] >= 0
    print(f"{top} {cls}: {len(hits)} rays, {hit.sum()} hit, instances {sorted(set(ids[hit]))}")
    assert 100 <= len(hits) <= 4096
    assert hit.sum() >= 16 and (~hit).sum() >= 16
    assert (ids[hit] >= 0).all() and (ids[~hit] == -1).all()


@pytest.mark.parametrize("top", ["stack64", "edges", "leaf8"])
def test_three_instances_are_hit_per_top_level(oracle, block, top):
    """`edges` and `leaf8`: in every mode (max_leaf, closest / any hit) on its own.  `stack64` is 64 copies of ONE placement: every ray
    that hits, hits all 64 at equal t, and which copy stands is decided by the order of the walk alone, the same for every ray; one mode
    reaches one or two ids, so there the count is taken over the modes together, which walk the copies in different orders."""
    seen = set()
    for max_leaf in E.MAX_LEAVES:
        for any_hit in (False, True):
            mode = set()
            for cls, tops in E.CLASSES.items():
                if top in tops:
                    ids = E.expect(oracle, block, top, max_leaf, cls, any_hit)[1]
                    mode |= set(ids[ids >= 0])
            print(top, max_leaf, any_hit, sorted(mode))
            assert top == "stack64" or len(mode) >= 3
            seen |= mode
    assert len(seen) >= 3


@pytest.mark.parametrize("top", E.CLASSES["b"])
def test_axis_rays_reach_zero_negative_zero_and_tiny_components(oracle, block, top):
    rays = E.rays_of(oracle, block, top, "b")
    counts = {"zero": 0, "negative zero": 0, "tiny": 0}
    for calls in E.entered(oracle, E.scene(block, top), rays):
        accepted = [d for d, ok, _ in calls if ok]
        if accepted:
            d = accepted[-1]                                             # the instance whose hit stands
            counts["zero"] += bool(((d == 0) & ~np.signbit(d)).any())
            counts["negative zero"] += bool(((d == 0) & np.signbit(d)).any())
            counts["tiny"] += bool(((d != 0) & (np.abs(d) < TINY)).any())
    print(top, counts)
    assert min(counts.values()) >= 16, counts


def test_face_rays_are_culled_both_ways(oracle, block):
    rays, graze = E.class_d(block, "one")
    calls = E.entered(oracle, E.scene(block, "one"), rays[graze])
    culled = sum(not c for c in calls)
    print(f"{culled} of {len(graze)} face rays culled")
    assert culled >= 8 and len(graze) - culled >= 8


def test_leaf_of_eight(oracle, block):
    """Under max_leaf 8 `leaf8` is ONE leaf: any-hit rays are accepted in its middle, closest hits stand in its first and its marked one."""
    sc = E.scene(block, "leaf8", 8)
    assert len(sc.tlas) == 1 and (sc.inst["instance_id"][:7] >= 0).all() and sc.inst["instance_id"][7] < 0
    closest, any_ = set(), set()
    for cls in ("e", "f"):
        for any_hit, into in ((False, closest), (True, any_)):
            ids = E.expect(oracle, block, "leaf8", 8, cls, any_hit)[1]
            into |= set(sc.slot[ids[ids >= 0]])
    assert {0, 7} <= closest and any_ & {2, 3, 4, 5}


# ---- the renderer's scene under the three matrix sets ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_hierarchy(native_build, tmp_path_factory):
    import instanced_scene_model as IM
    from conftest import GOLDEN
    from rodent_amd import instances as I
    scene = I.concat_scenes(IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("instanced_edges")))
    assert tuple(IM.placements()[1]) == E.SCENE_OBJECT_IDS
    return IM.object_bvhs(scene, scene.ranges)


@pytest.mark.parametrize("name", sorted(E.SCENE_BOX_TARGET))
def test_scene_classes_are_not_vacuous(oracle, scene_hierarchy, name):
    """Per matrix set and class: hits and misses; class b reaches zeros, negative zeros and tiny components in the instance whose hit
    stands; the face rays of class d are culled by the target's leaf box both ways; three instances are hit."""
    nodes, tris, table = scene_hierarchy
    transforms = E.scene_matrix_sets()[name]
    tlas, inst, info = M.build_tlas(nodes, table, M.descriptors(transforms, E.SCENE_OBJECT_IDS), 1)
    assert info[2] == 0
    model = (tlas, inst, nodes, tris)
    classes, graze = E.scene_edge_rays(oracle, name, transforms, model)
    assert "".join(classes) == E.SCENE_CLASSES
    seen = set()
    for cls, rays in classes.items():
        hits, ids = M.trace(oracle, *model, rays)
        hit = hits["tri_id"] >= 0
        print(f"{name} {cls}: {len(rays)} rays, {hit.sum()} hit, instances {sorted(set(ids[hit]))}")
        assert hit.sum() >= 16 and (~hit).sum() >= 16, (name, cls)
        seen |= set(ids[hit])
    assert len(seen) >= 3
    counts = {"zero": 0, "negative zero": 0, "tiny": 0}
    for calls in E.entered(oracle, model, classes["b"]):
        accepted = [d for d, ok, _ in calls if ok]
        if accepted:
            d = accepted[-1]
            counts["zero"] += bool(((d == 0) & ~np.signbit(d)).any())
            counts["negative zero"] += bool(((d == 0) & np.signbit(d)).any())
            counts["tiny"] += bool(((d != 0) & (np.abs(d) < TINY)).any())
    print(name, counts)
    assert min(counts.values()) >= 16, counts
    face = classes["d"][graze]
    slot = int(np.flatnonzero((inst["instance_id"] & 0x7FFFFFFF) == E.SCENE_BOX_TARGET[name])[0])
    o_org, o_dir = M._object_rays(inst[slot:slot + 1], face)
    into = [any(np.array_equal(d, o_dir[k, 0]) and np.array_equal(o, o_org[k, 0]) for d, _, o in calls)
            for k, calls in enumerate(E.entered(oracle, model, face))]
    print(f"{name}: {sum(into)} of {len(face)} face rays enter the target")
    assert sum(into) >= 8 and len(face) - sum(into) >= 8


# ---- the independent check ----------------------------------------------------------------------------------------------------------------
def mt_two_closest(tri_sets, rays):
    """Float64 Moeller-Trumbore (tests/test_oracle.py::mt_float64's) over every triangle: the closest and the second closest t."""
    v0, v1, v2 = (np.concatenate([t[k] for t in tri_sets]) for k in range(3))
    o, d = rays["org"].astype(np.float64)[:, None, :], rays["dir"].astype(np.float64)[:, None, :]
    e1, e2 = (v1 - v0)[None], (v2 - v0)[None]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        s = o - v0[None]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1)
        v = (d * q).sum(-1) * inv
        t = (e2 * q).sum(-1) * inv
        eps = 1e-9
        ok = (np.abs(det) > 0) & (u >= -eps) & (v >= -eps) & (u + v <= 1 + eps)
        ok &= (t >= rays["tmin"][:, None]) & (t <= rays["tmax"][:, None])
    t = np.sort(np.where(ok, t, np.inf), axis=1)
    return t[:, 0], t[:, 1]


def world_triangles(sc):
    """Per instance (v0, v1, v2) float64 of its object's triangles under the fp64 matrix."""
    out, seen = [], set()
    for k in range(sc.top.n):
        key = (sc.top.transforms[k].tobytes(), int(sc.top.obj[k]))      # coincident instances: the same triangles, once
        if key in seen:
            continue
        seen.add(key)
        row = sc.table[sc.top.obj[k]]
        tris = sc.tris[row["tri_offset"]: row["tri_offset"] + row["num_tris"]]
        m = sc.top.transforms[k].reshape(3, 4).astype(np.float64)
        v0 = tris["v0"].astype(np.float64)
        corners = (v0, v0 - tris["e1"].astype(np.float64), v0 + tris["e2"].astype(np.float64))
        out.append(tuple(c @ m[:, :3].T + m[:, 3] for c in corners))
    return out


# (class b has no ordinary rays: every one of its rays has a zero or tiny component; `stack64` is `pair`'s geometry)
@pytest.mark.parametrize("top,cls", [c for c in E.CASES if c[0] != "stack64" and c[1] != "b"])
def test_ordinary_rays_against_float64_moeller_trumbore(oracle, block, top, cls):
    sc = E.scene(block, top)
    rays = E.rays_of(oracle, block, top, cls).copy()
    if cls == "e":
        rays["tmax"] = E.FLT_MAX
    hits, _ = M.trace(oracle, *sc.model(), rays)
    # (|d| >= 1e-8 in world space too: the TLAS takes the same reciprocal of the world ray)
    ordinary = np.isfinite(rays["tmin"]) & np.isfinite(rays["tmax"]) & ~E.non_finite(rays)[1] & (np.abs(rays["dir"]) >= TINY).all(1)
    for k, calls in enumerate(E.entered(oracle, sc, rays)):
        if ordinary[k] and any((np.abs(d) < TINY).any() for d, _, _ in calls):
            ordinary[k] = False
    rays, hits = rays[ordinary], hits[ordinary]
    t, second = mt_two_closest(world_triangles(sc), rays)
    brute = np.zeros(len(rays), F.HIT1)
    brute["tri_id"], brute["t"] = np.where(np.isfinite(t), 0, -1), t
    with np.errstate(all="ignore"):
        amb = ambiguous_mask(brute, second)
    print(f"{top} {cls}: {len(rays)} ordinary rays, {np.isfinite(t).sum()} hit, ambiguous share {amb.mean():.4f}")
    assert len(rays) >= 16 and amb.mean() <= AMBIGUOUS_CAP
    keep = ~amb
    assert np.array_equal(hits["tri_id"][keep] >= 0, np.isfinite(t)[keep])
    both = keep & np.isfinite(t)
    assert np.allclose(hits["t"][both], t[both], rtol=1e-4, atol=0)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
CATCHES = {"fused": ("edges", "e", False), "strict_accept": ("pair", "f", False), "near_child_le": ("stack64", "f", False),
           "quiet_nan": ("one", "a", False)}


@pytest.mark.parametrize("name", sorted(CATCHES))
def test_a_perturbed_model_changes_expected_records(oracle, block, monkeypatch, name):
    top, cls, any_hit = CATCHES[name]
    leaves = E.MAX_LEAVES
    before = [E.expect(oracle, block, top, m, cls, any_hit) for m in leaves]
    attribute, replacement = E.perturbations()[name]
    monkeypatch.setattr(M, attribute, replacement)
    after = [E.expect(oracle, block, top, m, cls, any_hit) for m in leaves]
    changed = sum(int(((b[0].view("<u4").reshape(-1, 4) != a[0].view("<u4").reshape(-1, 4)).any(1) | (b[1] != a[1])).sum())
                  for b, a in zip(before, after))
    print(f"{name}: {changed} records of class {cls} on `{top}` change")
    assert changed >= 1


def test_dropping_copysign_changes_what_a_ray_enters_and_no_record(oracle, block, monkeypatch):
    """(the module's docstring)  The flat object in the plane z = 0 under the identity has a world box that is not widened across the
    plane (every term of e is 0); a ray 1 ... 3 denormal steps beside the plane with d_z = -0 has FLT_MAX * 1e-45 ~ 5e-7 as its slab
    distances, of a sign that only copysign decides."""
    pair = M.flat_object(0.0)
    nodes, tris, table = M.pack([pair])
    tlas, inst, info = M.build_tlas(nodes, table, M.descriptors(E.IDENTITY[None], [0]), 1)
    assert info[2] == 0 and list(tlas[0]["bounds"][4:6]) == [0, 0]
    org = np.float32([[-0.5, 0.1 * k - 0.3, 0] for k in range(6)])
    org[:, 2] = np.array([1, 2, 3, 0x80000001, 0x80000002, 0x80000003], "<u4").view("<f4")
    rays = F.make_rays(org, np.tile(np.float32([1, 0.25, -0.0]), (6, 1)), 0.0, 1.0)
    assert np.signbit(rays["dir"][:, 2]).all()

    class Flat:
        def model(self):
            return tlas, inst, nodes, tris
    records = lambda: [E.expect(oracle, block, t, 1, c, False) for c in ("b", "d") for t in E.CLASSES[c]]
    before, records_before = [len(c) for c in E.entered(oracle, Flat(), rays)], records()
    monkeypatch.setattr(M, "make_ray", E.unsigned_make_ray)
    after = [len(c) for c in E.entered(oracle, Flat(), rays)]
    print(f"copysign: entered {before} -> {after}")
    assert before != after
    for (h0, i0), (h1, i1) in zip(records_before, records()):
        assert h0.tobytes() == h1.tobytes() and np.array_equal(i0, i1)


# ---- containment --------------------------------------------------------------------------------------------------------------------------
def contains_exact_image(m, lo, hi):
    """Whether instance_model.world_box(m, lo, hi) contains all 8 corner images, in exact rational arithmetic."""
    box = [Fraction(float(x)) for x in M.world_box(m, lo[None], hi[None])[0]]
    mm = [[Fraction(float(x)) for x in row] for row in np.asarray(m, np.float32).reshape(3, 4)]
    for corner in range(8):
        p = [Fraction(float((hi if corner >> a & 1 else lo)[a])) for a in range(3)]
        for a in range(3):
            image = mm[a][0] * p[0] + mm[a][1] * p[1] + mm[a][2] * p[2] + mm[a][3]
            if not box[2 * a] <= image <= box[2 * a + 1]:
                return False
    return True


def test_widened_boxes_contain_the_exact_corner_images(block):
    nodes, _, table = M.pack([block, M.flat_object()])
    boxes = [M.object_box(nodes[offset]) for offset in table["node_offset"]]          # the Cornell block's and the flat object's
    for name, m, _ in E.edge_matrices():
        for lo, hi in boxes:
            assert contains_exact_image(m, lo, hi), name
    for transforms in E.scene_matrix_sets().values():
        for m in transforms:
            for lo, hi in boxes:
                assert contains_exact_image(m, lo, hi)


def test_underflowing_products_are_pinned_as_not_contained():
    """Entries and coordinates ~ 1e-22: every product is far below 2^-126, the relative widening has no room for a denormal's absolute
    rounding error, and the box misses a corner (include/rodent_instances.h states the domain)."""
    rng = np.random.default_rng(22)
    misses = 0
    for _ in range(20):
        m = (rng.uniform(-1, 1, 12) * 1e-22).astype(np.float32)
        m[3::4] = 0                                                      # no translation: nothing lifts the sums out of the denormals
        a, b = (rng.uniform(-1, 1, 3) * 1e-22).astype(np.float32), (rng.uniform(-1, 1, 3) * 1e-22).astype(np.float32)
        misses += not contains_exact_image(m, np.fmin(a, b), np.fmax(a, b))
    print(f"{misses} of 20 boxes miss a corner")
    assert misses >= 15
    # the same draws at an ordinary scale are contained
    rng = np.random.default_rng(22)
    for _ in range(20):
        m = rng.uniform(-1, 1, 12).astype(np.float32)
        a, b = rng.uniform(-1, 1, 3).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)
        assert contains_exact_image(m, np.fmin(a, b), np.fmax(a, b))


# ---- flags and stack --------------------------------------------------------------------------------------------------------------------
def test_flag_boundary_of_the_inverse(block):
    nodes, _, table = M.pack([block])
    for k, flags in E.FLAG_BOUNDARY.items():
        m = E.place(np.eye(3) * 2.0 ** k)[None]
        assert np.isfinite(m).all() and m[0, 0] == np.float32(2.0 ** k) != 0
        assert M.build_tlas(nodes, table, M.descriptors(m, [0]), 1)[2][2] == flags, k
    w, bad = M.invert(E.place(np.eye(3) * 2.0 ** -127))
    assert not bad.any() and w[0, 0] == np.float32(2.0 ** 127)


def test_every_edge_matrix_is_accepted():
    named = E.edge_matrices()
    w, bad = M.invert(np.array([m for _, m, _ in named]))
    assert not bad.any()
    near = w[[n for n, _, _ in named].index("near_singular")]
    assert 9e5 < np.abs(near[[0, 1, 4, 5]]).min() and np.abs(near[[0, 1, 4, 5]]).max() < 1.1e6
    for name, exact in (("scale_2^-20", 2.0 ** 20), ("scale_2^20", 2.0 ** -20)):
        assert w[[n for n, _, _ in named].index(name)][0] == np.float32(exact)


@pytest.mark.parametrize("name", sorted(E.STACK_LAYOUTS))
def test_stack_layouts_land_on_their_side_of_the_limit(oracle, name):
    obj, tlas, inst, rays = E.stack_layout(name)
    nodes, tris, _ = M.pack([obj])
    p = M.peak(oracle, tlas, inst, nodes, tris, rays)
    what, levels, flagged = E.STACK_LAYOUTS[name]
    own = 0 if what == "flat" else 40
    assert set(p) == {0, levels + own}, sorted(set(p))
    assert (p.max() + 2 > 64) == flagged
    assert (p == 0).sum() >= 16 and (p > 0).sum() >= 64
