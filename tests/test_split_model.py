"""CPU checks of tests/split_model.py, the model the splitting device builder (rodent_hip_build_bvh2_tri1_split) is held to byte for
byte (tests/test_gpu_build_split.py): no budget (or one piece) is the optimising builder exactly; split trees are valid hierarchies
over references whose boxes still cover every point of every triangle; the allotment stays within its budget; on long diagonal
slivers the split tree's SAH cost drops; the oracle on split trees finds the brute-force hits."""
import numpy as np
import pytest

import lbvh_model as L
import split_model as SM
import trbvh_model as T
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_gpu_build_model import mesh
from test_gpu_build_opt_model import soup


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


def slivers(n, seed, spread=50.0):
    """Long thin triangles in random oblique directions (pipes, cables): boxes that are mostly empty."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 40, (n, 1)).astype(np.float32)
    w = rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
    return mesh(np.stack([a, a + d, a + d * np.float32(0.5) + w], 1))


def sliver_soup_with_unmade_splits(n=200, seed=3):
    """Over a frame of [0, 1024]^3 (unit grid cells), short diagonal slivers across the point (512, 512, 512): only the three level-9
    planes cross them, so their allotment of up to 4 extra pieces each cannot always be made (info[6] > 0)."""
    rng = np.random.default_rng(seed)
    corner = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1024, 1024, 1024], [1023, 1024, 1024], [1024, 1023, 1024]]])
    c = np.float32(512) + rng.uniform(-0.05, 0.05, (n, 1, 3)).astype(np.float32)
    d = rng.uniform(0.2, 0.45, (n, 1, 3)).astype(np.float32) * rng.choice([-1, 1], (n, 1, 3)).astype(np.float32)
    w = rng.normal(size=(n, 1, 3)).astype(np.float32) * np.float32(0.01)
    return mesh(np.concatenate([corner, np.concatenate([c - d, c + d, c + w], 1)]))


def cases(cornell_scene):
    out = {"cornell": (cornell_scene.vertices, cornell_scene.indices)}
    out.update({f"soup{n}": soup(n, n) for n in (1, 2, 3, 8, 65, 1001)})
    out["slivers"] = slivers(1500, 1)
    return out


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2][:4], b[2][:4])


@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_no_budget_or_one_piece_is_the_unsplit_builder(cornell_scene, passes):
    for name, (v, ix) in cases(cornell_scene).items():
        for max_leaf in (1, 2, 8):
            ref = T.build(v, ix, max_leaf, passes) if passes else L.build(v, ix, max_leaf)
            for budget, pieces in ((0.0, 64), (4.0, 1), (0.0, 1)):
                got = SM.build(v, ix, max_leaf, passes, budget, pieces)
                assert same(got, ref), (name, max_leaf, budget, pieces)
                assert list(got[2][4:]) == [len(ix), 0, 0, 0]


def record_boxes(stats, nodes, tris):
    return SM.leaf_boxes_of_records(nodes, tris)


def covered(points, boxes):
    """Per point [k, 3] (float64): inside some of `boxes` [m, 6] (float32 compared exactly in float64)?"""
    b = boxes.astype(np.float64)
    inside = ((points[:, None, 0::1] >= b[None, :, 0::2]) & (points[:, None, :] <= b[None, :, 1::2])).all(-1)
    return inside.any(1)


@pytest.mark.parametrize("budget, pieces", [(1.0, 64), (4.0, 64), (4.0, 3)])
def test_leaf_boxes_cover_every_point_of_every_triangle(budget, pieces):
    rng = np.random.default_rng(11)
    for v, ix in (slivers(800, 2), sliver_soup_with_unmade_splits(), soup(500, 4)):
        st = {}
        nodes, tris, info = SM.build(v, ix, 2, 3, budget, pieces, stats=st)
        SM.check_split_structure(nodes, tris, len(ix), 2, pieces)
        assert info[5] > 0
        leaf_of = SM.leaf_boxes_of_records(nodes, tris)
        ids = (tris["prim_id"] & 0x7FFFFFFF).astype(np.int64)
        corners = v[:, :3][ix[:, :3]].astype(np.float64)                       # [n, 3, 3]
        bary = rng.dirichlet((1, 1, 1), (len(ix), 16))
        edge = rng.uniform(0, 1, (len(ix), 8, 1))
        for t in range(len(ix)):
            p = corners[t]
            pts = np.concatenate([p, bary[t] @ p] + [p[i] + edge[t] * (p[(i + 1) % 3] - p[i]) for i in range(3)])
            pts = np.clip(pts, p.min(0), p.max(0))       # float64 rounding of a sample must not leave the vertices' own range
            assert covered(pts, leaf_of[ids == t]).all(), t
            refb = st["refbox"][st["reftri"] == t]
            assert covered(pts, refb).all(), t
            tb = st["tbox"][t]
            assert (refb[:, 0::2] >= tb[0::2]).all() and (refb[:, 1::2] <= tb[1::2]).all()


def test_allotment_stays_within_the_budget():
    for v, ix in (slivers(2000, 5), sliver_soup_with_unmade_splits(), soup(1001, 1001)):
        for budget in (0.25, 1.0, 4.0):
            for pieces in (2, 8, 64):
                st = {}
                _, tris, info = SM.build(v, ix, 2, 0, budget, pieces, stats=st)
                s = st["s"]
                assert s.sum() <= st["B"] and s.max() <= pieces - 1
                assert info[4] == len(tris) <= SM.max_refs(len(ix), budget, pieces)
                assert info[4] + info[6] == len(ix) + s.sum()
    # the clamp at 2^25 references, on the allotment arithmetic alone
    n = (1 << 25) - 100
    assert SM.split_budget(n, 4.0) == 100 and SM.max_refs(n, 4.0, 64) == 1 << 25
    p = np.float32([3.0, 1.0, 0.0, 2.0, 3.0])
    w, W, s = SM.allot(p, 100, 64)
    assert list(w) == [65536, 21845, 0, 43690, 65536] and W == int(w.sum())
    assert s.sum() <= 100 and list(s) == [int(x) * 100 // W if int(x) * 100 // W < 63 else 63 for x in w]
    assert list(SM.allot(p, 100, 2)[2]) == [1, 1, 0, 1, 1]
    assert list(SM.allot(np.zeros(4, np.float32), 100, 64)[2]) == [0, 0, 0, 0]


def test_unmade_splits_are_counted():
    v, ix = sliver_soup_with_unmade_splits()
    st = {}
    nodes, tris, info = SM.build(v, ix, 2, 3, 4.0, 64, stats=st)
    assert info[6] > 0, "the input no longer leaves splits unmade"
    SM.check_split_structure(nodes, tris, len(ix), 2, 64)


@pytest.mark.parametrize("passes", [0, 3])
def test_split_slivers_lower_the_sah_cost(passes):
    v, ix = slivers(3000, 1)
    ref = SM.build(v, ix, 2, passes, 0.0)
    got = SM.build(v, ix, 2, passes, 1.0)
    assert got[2][4] > len(ix)
    base, split = L.sah_cost(ref[0], ref[1], T.NODE_COST, T.TRI_COST), L.sah_cost(got[0], got[1], T.NODE_COST, T.TRI_COST)
    print(f"slivers, {passes} passes: SAH {base:.1f} -> {split:.1f} with {got[2][4]} references")
    assert split < base


def test_flagged_triangles_are_not_split():
    v, ix = slivers(200, 7)
    v[5, 0] = np.nan
    ix[9, 1] = 10 ** 6
    st = {}
    nodes, tris, info = SM.build(v, ix, 2, 0, 4.0, 64, stats=st)
    assert info[2] == L.BAD_INDEX | L.NON_FINITE
    flagged = SM.triangle_flags(v, ix)
    assert (st["p"][flagged] == 0).all() and (st["s"][flagged] == 0).all() and np.isfinite(st["p"]).all()
    assert 0 < st["W"] < 1 << 63


def test_model_hits_agree_with_brute_force(oracle, cornell, cornell_scene):
    from rodent_amd import raygen
    lo, hi = np.float32([-60] * 3), np.float32([60] * 3)
    sets = [(cornell_scene.vertices, cornell_scene.indices, rays) for rays in cornell.ray_sets.values()]
    sets.append((*slivers(2000, 9), raygen.random_rays(lo, hi, 20000, 9, 0.0, 1.0)))
    for v, ix, rays in sets:
        rays = rays[(rays["dir"] != 0).all(axis=1)]
        for max_leaf, passes, budget in ((1, 0, 1.0), (2, 3, 1.0), (8, 3, 4.0)):
            nodes, tris, _ = SM.build(v, ix, max_leaf, passes, budget)
            SM.check_split_structure(nodes, tris, len(ix), max_leaf, 64, preorder=passes > 0)
            got, st = oracle.traverse(2, nodes, tris, rays)
            assert st["max_stack"] < 64
            sbvh_like = np.zeros(len(ix), tris.dtype)           # brute force over the triangles themselves, once each
            first = np.unique(tris["prim_id"] & 0x7FFFFFFF, return_index=True)[1]
            sbvh_like[:] = tris[first]
            brute, second = oracle.brute_force(sbvh_like, rays)
            amb = ambiguous_mask(brute, second)
            assert np.array_equal(got["tri_id"] >= 0, brute["tri_id"] >= 0)
            assert np.array_equal(got["tri_id"][~amb], brute["tri_id"][~amb])
            hit = brute["tri_id"] >= 0
            assert np.array_equal(got["t"][hit & ~amb], brute["t"][hit & ~amb])
