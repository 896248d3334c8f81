"""CPU checks of tests/lbvh_model.py, the model the device BVH builder is held to byte for byte (tests/test_gpu_build.py): its trees
are valid BVH2 / Tri1 hierarchies, their depth stays within 30 + ceil(log2 n) on adversarial inputs, they give the brute-force answers,
and their quality on the atrium is in the range an LBVH should have."""
import numpy as np
import pytest

import lbvh_model as L
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_builder import check_bvh2


def mesh(tri_vertices, geom=None):
    """[n, 3, 3] corners -> (vertices [3n, 4], indices [n, 4])."""
    t = np.asarray(tri_vertices, np.float32)
    n = len(t)
    v = np.zeros((3 * n, 4), np.float32)
    v[:, :3] = t.reshape(-1, 3)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    if geom is not None:
        ix[:, 3] = geom
    return v, ix


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


@pytest.mark.parametrize("max_leaf", [1, 2, 4, 8])
def test_model_trees_are_valid(cornell_scene, max_leaf):
    rng = np.random.default_rng(max_leaf)
    cases = [(cornell_scene.vertices, cornell_scene.indices)] + [mesh(rng.uniform(-5, 5, (n, 3, 3))) for n in (1, 2, 3, 9, 64, 65, 4097)]
    for v, ix in cases:
        nodes, tris, info = L.build(v, ix, max_leaf)
        check_bvh2(nodes, tris, len(ix))
        assert info[0] == len(nodes) and info[2] == 0
        assert len(nodes) <= max(1, len(ix) - 1)
        ends = np.nonzero(tris["prim_id"] < 0)[0]
        assert ends[-1] == len(tris) - 1 and (np.diff(np.concatenate([[-1], ends])) <= max_leaf).all()
        assert sorted(tris["prim_id"] & 0x7FFFFFFF) == list(range(len(ix)))


def tree_depth(nodes):
    depth, frontier, d = 0, [0], 0
    while frontier:
        d += 1
        depth = d
        c = nodes["child"][frontier]
        frontier = list(c[c > 0] - 1)
    return depth


@pytest.mark.parametrize("case", ["one_centroid", "flat"])
def test_depth_bound_on_adversarial_inputs(case):
    rng = np.random.default_rng(5)
    n = 100_000
    if case == "one_centroid":
        # every triangle symmetric about the origin: one shared centroid, one Morton code; only the index tie-break splits them
        a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        t = np.stack([a, -a, np.zeros_like(a)], 1)
    else:
        t = rng.uniform(-100, 100, (n, 3, 3)).astype(np.float32)
        t[..., 1] = 3.0
    v, ix = mesh(t)
    nodes, tris, info = L.build(v, ix, 2)
    assert info[1] == tree_depth(nodes) <= L.depth_bound(n), (info[1], L.depth_bound(n))
    check_bvh2(nodes, tris, n)


def test_zero_extent_and_nan_inputs():
    v, ix = mesh(np.zeros((5, 3, 3), np.float32))                  # no extent on any axis: every code is 0
    nodes, tris, info = L.build(v, ix, 1)
    check_bvh2(nodes, tris, 5)
    assert list(tris["prim_id"] & 0x7FFFFFFF) == [0, 1, 2, 3, 4]
    v[4, 1] = np.nan
    assert L.build(v, ix, 2)[2][2] == L.NON_FINITE
    ix[2, 0] = len(v)
    assert L.build(v, ix, 2)[2][2] == L.NON_FINITE | L.BAD_INDEX


def test_model_hits_agree_with_brute_force(oracle, cornell, cornell_scene):
    rng = np.random.default_rng(3)
    soup = mesh(rng.uniform(-5, 5, (3000, 3, 3)))
    lo, hi = np.float32([-5] * 3), np.float32([5] * 3)
    from rodent_amd import raygen
    sets = [(cornell_scene.vertices, cornell_scene.indices, rays) for rays in cornell.ray_sets.values()]
    sets.append((*soup, raygen.random_rays(lo, hi, 20000, 9, 0.0, 1.0)))
    for v, ix, rays in sets:
        # axis-parallel rays graze box faces, where a traversal legitimately differs from a box-free search (test_oracle.py)
        rays = rays[(rays["dir"] != 0).all(axis=1)]
        for max_leaf in (1, 2, 8):
            nodes, tris, _ = L.build(v, ix, max_leaf)
            got, _ = oracle.traverse(2, nodes, tris, rays)
            brute, second = oracle.brute_force(tris, rays)
            amb = ambiguous_mask(brute, second)
            assert np.array_equal(got["tri_id"] >= 0, brute["tri_id"] >= 0)
            assert np.array_equal(got["tri_id"][~amb], brute["tri_id"][~amb])
            hit = brute["tri_id"] >= 0
            assert np.allclose(got["t"][hit], brute["t"][hit], rtol=1e-4)


def test_atrium_camera_ray_steps_against_the_sbvh(oracle, tmp_path):
    from rodent_amd import raygen, scenes
    sc = S.convert(scenes.scene_obj("atrium"), tmp_path / "atrium.rscene")
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    rays = raygen.primary_rays(eye, d, up, fov, 256, 256, 0.0, scenes.PRIMARY_TMAX)
    nodes, tris, info = L.build(sc.vertices, sc.indices, 2)
    assert info[1] <= L.depth_bound(sc.num_tris)
    lbvh = oracle.ray_steps(nodes, tris, rays).sum(1).mean()
    sbvh = oracle.ray_steps(sc.nodes, sc.tris, rays).sum(1).mean()
    print(f"atrium camera rays, oracle steps per ray: LBVH {lbvh:.1f}, SBVH {sbvh:.1f} ({lbvh / sbvh:.2f} x); "
          f"SAH cost {L.sah_cost(nodes, tris):.1f} / {L.sah_cost(sc.nodes, sc.tris):.1f}")
    assert lbvh <= 2.5 * sbvh
