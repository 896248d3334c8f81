"""tests/motion_bvh_edge_fixtures.py is not vacuous (CPU only): every ray class holds hits and misses by the model alone, the model equals
a brute force over all triangles at the ray's time on the ordinary rays, the kernel's corners lie in the interpolated widened boxes in
exact rational arithmetic, each named perturbation of the model shows in the expectations, and the face rays of class d are culled on
one side of a face and taken on the other.

Three properties of these tests that follow from the arithmetic:
* class b cannot hit on `far`, `still` and `huge`: a zero or tiny direction component has the reciprocal +-FLT_MAX, the origin's product
  with it overflows for any coordinate beyond (-1, 1), and the slab test then fails at the root (instance_edge_fixtures states the same
  for the static kernels).  There the class is pinned as misses only; on every other shape its rays start where the two other
  coordinates lie inside (-0.9, 0.9).
* the `tiny` shapes have one to three triangles; a ray that starts inside the one leaf box in a random direction (class d) seldom sees
  them, so their lower bound is TINY_BOUND hits, not 16.
* an empty slot that is taken ends the walk (its child word is the word that ends a traversal), which oracle.binding cannot be asked to
  do; motion_bvh_edge_fixtures.EmptySlotTaken states what follows for a one-node tree.
"""
import numpy as np
import pytest

import motion_bvh_edge_fixtures as X
import motion_bvh_model as MB
from rodent_amd import formats as F
from test_motion_bvh_model import corners_outside, leaf_records, single_leaf

F32 = np.float32
AMBIGUOUS_CAP = 0.05
TINY_BOUND = 8
OVERFLOW_CULLED = ("far", "still", "huge")


def differing(a, b):
    return int((a.view("<u4").reshape(-1, 4) != b.view("<u4").reshape(-1, 4)).any(1).sum())


# ---- class counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", X.CASES)
def test_every_class_hits_and_misses(oracle, name, cls):
    rays, times = X.rays_of(oracle, name, cls)
    on = MB.traced(times)
    assert 100 <= len(rays) <= 1100 and len(set(times.view("<u4").tolist())) >= 3
    for max_leaf in X.MAX_LEAVES[name]:
        hits = X.expect(oracle, name, max_leaf, cls, False)
        hit = hits["tri_id"] >= 0
        print(f"{name} max_leaf {max_leaf} {cls}: {len(rays)} rays, {on.sum()} traced, {hit.sum()} hit, {(~hit & on).sum()} traced misses")
        assert not hit[~on].any() and hits["t"][~on].tobytes() == rays["tmax"][~on].tobytes()
        assert (~hit & on).sum() >= 16
        if cls == "b" and name in OVERFLOW_CULLED:
            assert hit.sum() == 0                                       # pinned: see the module's docstring
        else:
            assert hit.sum() >= (TINY_BOUND if name in X.TINY else 16)


def test_the_trees_with_an_empty_slot():
    """One leaf beside an empty slot: `tiny1` under every max_leaf, `tiny2` under 2 and 8, `tiny3` under 8; the fuse leaves the slot's
    (+inf, -inf) as it is at both keys, and the model walks key 0's there at every time."""
    empty = [(name, m) for name in X.TINY for m in X.MAX_LEAVES[name] if X.has_empty_slot(name, m)]
    assert empty == [("tiny1", 1), ("tiny1", 2), ("tiny1", 8), ("tiny2", 2), ("tiny2", 8), ("tiny3", 8)]
    for name, m in empty:
        mn, mt = X.records(name, m)
        assert len(mn) == 1 and mn["child"][0].tolist() == [~0, 0]
        for key in ("bounds0", "bounds1"):
            assert mn[key][0, 6:].tolist() == [np.inf, -np.inf] * 3
        for t in F32([0.0, 1.0, 0.5]):
            assert MB.at_time(mn, mt, t)[0]["bounds"][0, 6:].tolist() == [np.inf, -np.inf] * 3
        with np.errstate(invalid="ignore"):
            assert np.isnan(MB.lerp(mn["bounds0"][0, 6:], mn["bounds1"][0, 6:], F32(0))).all()       # what the kernel's registers hold


def test_the_collapsing_groups_collapse():
    """Group 1 is a line at t = 0.5 exactly (a zero normal from exact products) and of either orientation beside it; group 2 is a point
    at t = 1; group 3 changes its orientation between the keys."""
    mn, mt = X.records("collapsing", 2)
    prim = mt["key0"]["prim_id"] & 0x7FFFFFFF

    def normals(t):
        tris = MB.at_time(mn, mt, t)[1]
        return np.cross(tris["e1"].astype(np.float64), tris["e2"].astype(np.float64))
    g1, g2, g3 = prim < 16, (prim >= 16) & (prim < 32), (prim >= 32) & (prim < 48)
    assert not normals(X.HALF)[g1].any()
    before, after = normals(X.BESIDE_HALF[0])[g1], normals(X.BESIDE_HALF[1])[g1]
    assert (np.abs(before).max(1) > 0).all() and ((before * after).sum(1) < 0).all()
    assert not normals(F32(1))[g2].any() and (np.abs(normals(F32(0))[g2]).max(1) > 0).all()
    assert ((normals(F32(0))[g3] * normals(F32(1))[g3]).sum(1) < 0).all()


def test_garbage_words_change_no_hit(oracle):
    clean, garbage = X.records("far", 2), X.records(X.GARBAGE, 2)
    assert (garbage[0]["pad"] == X.PAD_GARBAGE).all() and all((garbage[1]["key1"][w] == -1).all() for w in MB.WORDS)
    assert garbage[0]["child"].tobytes() == clean[0]["child"].tobytes() and garbage[1]["key0"].tobytes() == clean[1]["key0"].tobytes()
    for cls in X.CLASSES:
        for any_hit in (False, True):
            assert X.expect(oracle, X.GARBAGE, 2, cls, any_hit).tobytes() == X.expect(oracle, "far", 2, cls, any_hit).tobytes()


# ---- the model against a brute force --------------------------------------------------------------------------------------------------------
def brute_force(oracle, mn, mt, rays, times):
    """(hits, ambiguous): the oracle over ONE leaf of all triangles at each ray's time, and the rays whose closest t two triangles share."""
    hits, tie = np.zeros(len(rays), F.HIT1), np.zeros(len(rays), bool)
    for t, sel in MB.time_groups(times):
        tris = MB.at_time(mn, mt, t)[1]
        hits[sel] = oracle.traverse(2, *single_leaf(tris), rays[sel])[0]
        whole = rays[sel].copy()
        whole["tmax"] = X.FLT_MAX                                          # (the second t of a ray that ends at its hit is its tmax)
        first, second = oracle.brute_force(tris, whole)
        tie[sel] = (first["tri_id"] >= 0) & (second == first["t"])
    return hits, tie


@pytest.mark.parametrize("name,cls", [c for c in X.CASES if c[1] != "b"])          # (every ray of class b has a zero or tiny component)
def test_ordinary_rays_equal_the_brute_force_at_the_rays_time(oracle, name, cls):
    rays, times = X.rays_of(oracle, name, cls)
    keep = X.ordinary(rays) & MB.traced(times)
    assert keep.sum() >= 16
    for max_leaf in X.MAX_LEAVES[name]:
        mn, mt = X.records(name, max_leaf)
        got = X.expect(oracle, name, max_leaf, cls, False)[keep]
        brute, tie = brute_force(oracle, mn, mt, rays[keep], times[keep])
        print(f"{name} max_leaf {max_leaf} {cls}: {keep.sum()} ordinary rays, {(brute['tri_id'] >= 0).sum()} hit, ambiguous share {tie.mean():.4f}")
        assert tie.mean() <= AMBIGUOUS_CAP
        assert got["t"].tobytes() == brute["t"].tobytes()
        assert np.array_equal(got["tri_id"] >= 0, brute["tri_id"] >= 0)
        assert got[~tie].tobytes() == brute[~tie].tobytes()
        assert MB.peak(oracle, mn, mt, rays, times).max() <= 63


# ---- containment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far", "small", "huge", "still", "collapsing"])
def test_kernel_corners_lie_in_the_interpolated_widened_box(name):
    sh = X.SHAPE[name]
    traced = X.palette()[MB.traced(X.palette())]
    k0, k1 = sh.v0[:, :3].reshape(sh.n, 9), sh.v1[:, :3].reshape(sh.n, 9)
    checks, bad = corners_outside(*leaf_records(k0, k1, MB.WIDEN), traced)
    print(f"{name}: {checks} corner / axis checks at {len(traced)} times: {bad} outside")
    assert checks == sh.n * 9 * len(traced) and bad == 0


def test_without_the_widening_corners_leave_the_box_and_a_hit_is_lost(oracle):
    """`still` and `far` with the widening set to 0: the rational check finds corners outside their boxes, and the model over such records
    loses hits the brute force has."""
    traced = X.palette()[MB.traced(X.palette())]
    lost = 0
    for name in ("still", "far"):
        sh = X.SHAPE[name]
        checks, bad = corners_outside(*leaf_records(sh.v0[:, :3].reshape(sh.n, 9), sh.v1[:, :3].reshape(sh.n, 9), 0.0), traced)
        print(f"{name} with no widening: {bad} of {checks} corner / axis checks outside")
        assert bad >= 1
        mn, mt, _ = MB.build(*X.topology(name, 2), sh.v0, sh.v1, sh.ix, 0.0)
        for cls in "ade":
            rays, times = X.rays_of(oracle, name, cls)
            keep = X.ordinary(rays) & MB.traced(times)
            got = MB.trace(oracle, mn, mt, rays[keep], times[keep])
            brute, _ = brute_force(oracle, mn, mt, rays[keep], times[keep])
            gone = int(((brute["tri_id"] >= 0) & (got["t"] != brute["t"])).sum())
            print(f"{name} {cls} with no widening: {gone} of {(brute['tri_id'] >= 0).sum()} brute-force hits lost or moved")
            lost += gone
    assert lost >= 1


def test_the_static_tree_of_still_loses_hits_the_motion_records_keep(oracle):
    """What tests/test_gpu_motion_bvh_edges.py's static anchor leaves out, pinned: at times 0, 1 and -0 the model over `still` equals the
    brute force on every ray, and the oracle over the static tree differs from it on at most STATIC_LOST_CAP rays per class -- and on
    at least one, a ray of class d."""
    mn, mt = X.records("still", 2)
    total = 0
    for time in (0.0, 1.0, -0.0):
        for cls in X.CLASSES:
            rays, _ = X.rays_of(oracle, "still", cls)
            static, brute, lost = X.static_anchor(oracle, rays, time)
            moving = MB.trace(oracle, mn, mt, rays, np.full(len(rays), time, F32))
            assert moving["t"].tobytes() == brute["t"].tobytes()
            assert lost.sum() <= X.STATIC_LOST_CAP and (brute["tri_id"][lost] >= 0).all()
            assert (cls == "d") == bool(lost.any())
            total += int(lost.sum())
    print(f"still: the static tree loses {total} brute-force hits over 3 times x 5 classes")
    assert total >= 1


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
# perturbation: the (shape, class) pairs whose expectations (closest hit, every max_leaf of the shape) are compared
CATCHES = {"fused": [("far", "e"), ("collapsing", "e"), ("huge", "e")],
           "one_product": [("far", "e"), ("collapsing", "e"), ("huge", "e")],
           "one_refused": [("small", "a"), ("tiny1", "c")],
           "negative_zero_refused": [("small", "a"), ("tiny1", "c")],
           "clamped": [("small", "a"), ("tiny1", "c")],
           "key1_words": [(X.GARBAGE, "a"), (X.GARBAGE, "e")]}


def expectations(oracle, cases):
    return [X.expect(oracle, name, m, cls, False) for name, cls in cases for m in X.MAX_LEAVES.get(name, (2,))]


@pytest.mark.parametrize("name", sorted(CATCHES))
def test_a_perturbed_model_changes_expected_records(oracle, monkeypatch, name):
    before = expectations(oracle, CATCHES[name])
    for attribute, replacement in X.perturbations()[name].items():
        monkeypatch.setattr(MB, attribute, replacement)
    after = expectations(oracle, CATCHES[name])
    changed = [differing(b, a) for b, a in zip(before, after)]
    print(f"{name}: {changed} records change on {CATCHES[name]}")
    assert min(changed) >= 1 if name in ("one_refused", "negative_zero_refused", "clamped", "key1_words") else sum(changed) >= 1


def test_an_empty_slot_that_is_taken_changes_expected_records(oracle):
    taken = X.EmptySlotTaken(oracle)
    for name in X.TINY:
        for max_leaf in X.MAX_LEAVES[name]:
            changed = sum(differing(X.expect(oracle, name, max_leaf, cls, False), X.expect(taken, name, max_leaf, cls, False))
                          for cls in X.CLASSES)
            print(f"empty slot taken: {changed} records change on {name} under max_leaf {max_leaf}")
            assert (changed >= 16) == X.has_empty_slot(name, max_leaf) and (changed == 0) != X.has_empty_slot(name, max_leaf)


# ---- class d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.TINY + ("small",))
def test_face_rays_are_culled_on_one_side_and_taken_on_the_other(oracle, name):
    """The rays parallel to a face of the leaf's box at their own time, against that box alone: the oracle's count of triangles a ray
    visits says whether the slab test let it in.  (Shapes whose boxes lie inside (-1, 1); elsewhere the overflow culls all of them.)"""
    max_leaf = X.MAX_LEAVES[name][-1]
    rays, times, graze = X.class_d(name, max_leaf)
    mn, mt = X.records(name, max_leaf)
    node, slot = map(int, np.argwhere(mn["child"] < 0)[0])
    into = culled = 0
    for t in X.D_TIMES:
        nodes, tris = MB.at_time(mn, mt, t)
        first = ~int(nodes["child"][node, slot])
        last = first + int(np.flatnonzero(tris["prim_id"][first:] < 0)[0])
        alone = single_leaf(tris[first: last + 1])
        alone[0]["bounds"][0, :6] = nodes["bounds"][node, 6 * slot: 6 * slot + 6]
        sel = graze[times[graze].view("<u4") == t.view("<u4")]
        assert len(sel) == 168
        visited = oracle.ray_steps(*alone, rays[sel])[:, 1] > 0
        into, culled = into + int(visited.sum()), culled + int((~visited).sum())
    print(f"{name}: {into} face rays enter the leaf box, {culled} are culled")
    assert into >= 24 and culled >= 24
