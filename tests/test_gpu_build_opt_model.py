"""CPU checks of tests/trbvh_model.py, the model the optimising device builder (treelet restructuring + SAH leaf collapse) is held to
byte for byte (tests/test_gpu_build_opt.py): its trees are valid BVH2 / Tri1 hierarchies with leaves of at most max_leaf triangles and
at most 56 levels, their SAH cost is no higher than the LBVH's, they give the brute-force answers, and on the atrium they need fewer
traversal steps per camera ray than the LBVH."""
import numpy as np
import pytest

import lbvh_model as L
import trbvh_model as T
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_gpu_build_model import mesh

MAX_LEAVES = (1, 2, 4, 8)
PASSES = (1, 2, 3)


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


def soup(n, seed):
    """Uniform triangles with degenerate ones (a point, a line) and shared centroids mixed in; a flat z axis when `seed` is odd."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-5, 5, (n, 3, 3)).astype(np.float32)
    if seed % 2:
        t[..., 2] = 1.5
    t[::7, 1], t[::7, 2] = t[::7, 0], t[::7, 0]
    t[3::11, 2] = t[3::11, 1]
    t[1::5] = t[0:-1:5][:, [0, 2, 1]][: len(t[1::5])]
    return mesh(t)


def adversarial(n=3000, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    one_centroid = np.stack([a, -a, np.zeros_like(a)], 1)          # one Morton code for all
    flat = rng.uniform(-100, 100, (n, 3, 3)).astype(np.float32)
    flat[..., 1] = 3.0
    coincident = np.repeat(rng.uniform(-1, 1, (1, 3, 3)).astype(np.float32), 200, 0)
    return {"one_centroid": mesh(one_centroid), "flat": mesh(flat), "coincident": mesh(coincident),
            "zero_extent": mesh(np.zeros((40, 3, 3), np.float32))}


def cases(cornell_scene):
    out = {"cornell": (cornell_scene.vertices, cornell_scene.indices)}
    out.update({f"soup{n}": soup(n, n) for n in (2, 3, 7, 8, 64, 65, 1001, 20000)})
    out.update(adversarial())
    return out


def check(v, ix, max_leaf, passes):
    nodes, tris, info = T.build(v, ix, max_leaf, passes)
    depth = T.check_structure(nodes, tris, len(ix), max_leaf)
    assert info[0] == len(nodes) and info[1] == depth and info[2] == 0
    ln, lt, _ = L.build(v, ix, max_leaf)
    opt, lbvh = L.sah_cost(nodes, tris, T.NODE_COST, T.TRI_COST), L.sah_cost(ln, lt, T.NODE_COST, T.TRI_COST)
    assert opt <= lbvh * (1 + 1e-5), (opt, lbvh)
    return nodes, tris, info


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_model_trees_are_valid_and_no_worse_than_the_lbvh(cornell_scene, max_leaf, passes):
    for name, (v, ix) in cases(cornell_scene).items():
        try:
            check(v, ix, max_leaf, passes)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


def test_passes_zero_is_the_lbvh(cornell_scene):
    for v, ix in cases(cornell_scene).values():
        for max_leaf in MAX_LEAVES:
            a, b = T.build(v, ix, max_leaf, 0), L.build(v, ix, max_leaf)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_single_triangle_and_collapsed_root():
    v, ix = soup(1, 2)
    nodes, tris, info = T.build(v, ix, 2, 2)
    assert list(info) == [1, 1, 0, 0] and T.check_structure(nodes, tris, 1, 2) == 1
    v, ix = mesh(np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0.01], [1, 0, 0.01], [0, 1, 0.01]]]))
    nodes, tris, info = T.build(v, ix, 2, 1)          # two overlapping triangles: one leaf beats a node over two leaves
    assert list(info) == [1, 1, 0, 0] and nodes[0]["child"].tolist() == [~0, 0]
    nodes, tris, info = T.build(v, ix, 1, 1)
    assert info[0] == 1 and nodes[0]["child"].tolist() == [~0, ~1]


def deep_input(n, seed, lo=-9, hi=3):
    """Triangles (a, -a, 0): one shared centroid (the Karras tree splits them by index alone), sizes over 10^lo ... 10^hi.  The SAH
    wants the big ones near the root and the small ones deep down, so the restructured tree runs into the depth rule."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32) * np.float32(10.0) ** rng.uniform(lo, hi, (n, 1)).astype(np.float32)
    return mesh(np.stack([a, -a, np.zeros_like(a)], 1))


@pytest.mark.parametrize("n, seed", [(20000, 13), (60000, 13)])
def test_depth_rule_rejects_topologies_and_holds(n, seed):
    v, ix = deep_input(n, seed)
    nodes, tris, info = T.build(v, ix, 1, 3)
    assert info[3] > 0, "the input no longer reaches the depth rule"
    assert info[1] == T.check_structure(nodes, tris, n, 1) <= T.MAX_DEPTH
    print(f"{n} triangles: depth {info[1]}, {info[3]} topologies rejected")


@pytest.mark.parametrize("slack", [0, 1, 2])
def test_depth_rule_holds_at_a_lower_limit(monkeypatch, slack):
    # the rule at a limit just above the Karras tree's own height: most treelets near the top are rejected, and the stored heights
    # of their roots must stay true for the ancestors (and for the model's level-by-level batches)
    for seed in (1, 2, 3):
        v, ix = deep_input(4000, seed, -12, 4)
        karras_depth = L.build(v, ix, 1)[2][1]
        monkeypatch.setattr(T, "MAX_DEPTH", int(karras_depth) + slack)
        for passes in PASSES:
            nodes, tris, info = T.build(v, ix, 1, passes)
            assert info[1] == T.check_structure(nodes, tris, len(ix), 1) <= T.MAX_DEPTH
            if passes == 3:
                assert info[3] > 0


def test_renderer_refuses_passes_without_a_device_hierarchy(cornell_scene):
    from rodent_amd import render as R
    with pytest.raises(ValueError, match="gpu_bvh"):
        R.Renderer(cornell_scene, 16, 16, gpu_bvh_passes=2)


def test_model_hits_agree_with_brute_force(oracle, cornell, cornell_scene):
    from rodent_amd import raygen
    rng = np.random.default_rng(3)
    soup3k = mesh(rng.uniform(-5, 5, (3000, 3, 3)))
    lo, hi = np.float32([-5] * 3), np.float32([5] * 3)
    sets = [(cornell_scene.vertices, cornell_scene.indices, rays) for rays in cornell.ray_sets.values()]
    sets.append((*soup3k, raygen.random_rays(lo, hi, 20000, 9, 0.0, 1.0)))
    for v, ix, rays in sets:
        rays = rays[(rays["dir"] != 0).all(axis=1)]
        for max_leaf, passes in ((1, 1), (2, 2), (8, 3)):
            nodes, tris, _ = T.build(v, ix, max_leaf, passes)
            T.check_structure(nodes, tris, len(ix), max_leaf)
            got, st = oracle.traverse(2, nodes, tris, rays)
            assert st["max_stack"] < 64
            brute, second = oracle.brute_force(tris, rays)
            amb = ambiguous_mask(brute, second)
            assert np.array_equal(got["tri_id"] >= 0, brute["tri_id"] >= 0)
            assert np.array_equal(got["tri_id"][~amb], brute["tri_id"][~amb])
            hit = brute["tri_id"] >= 0
            assert np.allclose(got["t"][hit], brute["t"][hit], rtol=1e-4)


def test_atrium_camera_ray_steps_drop_below_the_lbvh(oracle, tmp_path):
    from rodent_amd import raygen, scenes
    sc = S.convert(scenes.scene_obj("atrium"), tmp_path / "atrium.rscene")
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    rays = raygen.primary_rays(eye, d, up, fov, 256, 256, 0.0, scenes.PRIMARY_TMAX)
    ln, lt, _ = L.build(sc.vertices, sc.indices, 2)
    nodes, tris, info = T.build(sc.vertices, sc.indices, 2, 3)
    assert info[1] == T.check_structure(nodes, tris, sc.num_tris, 2)
    steps = {k: oracle.ray_steps(nn, tt, rays).sum(1).mean() for k, (nn, tt) in
             {"lbvh": (ln, lt), "opt": (nodes, tris), "sbvh": (sc.nodes, sc.tris)}.items()}
    sah = {k: L.sah_cost(nn, tt) for k, (nn, tt) in {"lbvh": (ln, lt), "opt": (nodes, tris), "sbvh": (sc.nodes, sc.tris)}.items()}
    print(f"atrium camera rays, oracle steps per ray: LBVH {steps['lbvh']:.1f}, 3 treelet passes {steps['opt']:.1f}, "
          f"SBVH {steps['sbvh']:.1f} (optimised / SBVH {steps['opt'] / steps['sbvh']:.2f} x); SAH cost {sah['lbvh']:.1f} / "
          f"{sah['opt']:.1f} / {sah['sbvh']:.1f}; depth {info[1]}, {info[3]} topologies rejected by the depth rule")
    assert steps["opt"] < steps["lbvh"]
