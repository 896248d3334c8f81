"""CPU checks of tests/ploc_model.py, the model the PLOC topology stage of the device builder (rodent_hip_build_bvh2_tri1_ploc,
include/rodent_build.h) is held to byte for byte (tests/test_gpu_build_ploc.py): its vectorised clustering equals a plain per-cluster
loop of the same rule, its trees are valid BVH2 / Tri1 hierarchies, the xor tie rule keeps identical triangles balanced, the depth limit
holds, it composes with the split front, and on the atrium it reaches the costs the rule was chosen for."""
import numpy as np
import pytest

import lbvh_model as L
import ploc_model as P
import split_model as SP
import trbvh_model as T
from conftest import GOLDEN
from rodent_amd import scene as S
from test_gpu_build_model import mesh
from test_gpu_build_opt_model import soup

F32 = np.float32
RADII = (1, 8, 64)
SIZES = (1, 2, 3, 5, 17, 257, 1000)


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


def sorted_refs(v, ix):
    tv, geom, _ = L.load_triangles(v, ix)
    return L.sort_references(tv, geom, *L.triangle_references(tv))


def area(b):
    dx, dy, dz = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    return (dx * dy + dy * dz) + dz * dx


def cluster_loop(leafbox, radius, depth_limit=0):
    """The rule of include/rodent_build.h, cluster by cluster in plain Python: what ploc_model.cluster returns."""
    n = len(leafbox)
    m = n - 1
    D = depth_limit or 56
    I = 4 * P.clog2(n) + 8
    clusters = [(m + p, [F32(x) for x in leafbox[p]], 0) for p in range(n)]
    left, right, parent = np.zeros(m, np.int64), np.zeros(m, np.int64), np.full(m + n, -1, np.int64)
    t = 0
    while len(clusters) > 1:
        C = len(clusters)
        choice = []
        for i in range(C):
            if t >= I:
                choice.append(i ^ 1 if i ^ 1 < C else -1)
                continue
            best, key = -1, None
            _, bi, hi = clusters[i]
            for j in range(max(0, i - radius), min(C - 1, i + radius) + 1):
                _, bj, hj = clusters[j]
                if j == i or 1 + max(hi, hj) > D - P.clog2(C):
                    continue
                d = area([min(bi[k], bj[k]) if k % 2 == 0 else max(bi[k], bj[k]) for k in range(6)])
                if d != d:
                    continue
                if key is None or d < key[0] or (d == key[0] and (i ^ j) < key[1]):
                    best, key = j, (d, i ^ j)
            choice.append(best)
        out, leaders = [], 0
        for i in range(C):
            j = choice[i]
            if j >= 0 and choice[j] == i:
                if i < j:
                    (a, ba, ha), (b, bb, hb) = clusters[i], clusters[j]
                    node = (C - 2) - leaders
                    leaders += 1
                    left[node], right[node], parent[a], parent[b] = a, b, node, node
                    out.append((node, [min(ba[k], bb[k]) if k % 2 == 0 else max(ba[k], bb[k]) for k in range(6)], 1 + max(ha, hb)))
            else:
                out.append(clusters[i])
        clusters = out
        t += 1
    return left, right, parent, t


def meshes(cornell_scene):
    out = {"cornell": (cornell_scene.vertices, cornell_scene.indices)}
    out.update({f"soup{n}-{seed}": soup(n, seed) for n in SIZES for seed in (n, n + 1)})
    return out


@pytest.mark.parametrize("radius", RADII)
def test_model_equals_a_plain_loop_of_the_rule(cornell_scene, radius):
    with np.errstate(all="ignore"):
        for name, (v, ix) in meshes(cornell_scene).items():
            if len(ix) < 2:
                continue
            leafbox = sorted_refs(v, ix)[1]
            got, want = P.cluster(leafbox, radius), cluster_loop(leafbox, radius)
            assert got[3] == want[3], name
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])), name
            assert got[2][0] == -1 and sorted(np.concatenate([got[0], got[1]])) == [k for k in range(2 * len(ix) - 1) if k != 0], name


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("max_leaf, passes", [(1, 0), (2, 1), (4, 0), (8, 3)])
def test_model_trees_are_valid(cornell_scene, radius, max_leaf, passes):
    for name, (v, ix) in meshes(cornell_scene).items():
        nodes, tris, info = P.build(v, ix, max_leaf, passes, radius)
        depth = T.check_structure(nodes, tris, len(ix), max_leaf)
        assert (info[0], info[1], info[2], info[4]) == (len(nodes), depth, 0, len(ix)), name
        # the flat soups converge slowly at radius 64 (chains of equal areas): some do reach the forced iterations
        assert info[5] == info[6] == 0 and 0 <= info[7] <= P.nn_iterations(len(ix)) + P.clog2(len(ix)), name
        assert (info[7] == 0) == (len(ix) == 1), name


def test_single_triangle_is_the_single_leaf():
    v, ix = soup(1, 2)
    nodes, tris, info = P.build(v, ix, 2, 0, 8)
    assert list(info) == [1, 1, 0, 0, 1, 0, 0, 0] and nodes[0]["child"].tolist() == [~0, 0]
    ln, lt, _ = L.build(v, ix, 2)
    assert nodes.tobytes() == ln.tobytes() and tris.tobytes() == lt.tobytes()


@pytest.mark.parametrize("radius", RADII)
def test_identical_triangles_pair_up_instead_of_chaining(radius):
    one = np.random.default_rng(1).uniform(-1, 1, (1, 3, 3)).astype(F32)
    v, ix = mesh(np.repeat(one, 300, 0))
    leafbox = sorted_refs(v, ix)[1]
    t, iterations = P.fitted(leafbox, 1, 0, radius)
    assert t.height[0] <= P.clog2(300) + 1, t.height[0]
    nodes, tris, info = P.build(v, ix, 1, 0, radius)
    assert info[1] == T.check_structure(nodes, tris, 300, 1) <= P.clog2(300) + 1
    assert info[7] == iterations <= P.nn_iterations(300)


@pytest.mark.parametrize("n", [64, 1000])
def test_depth_limit_holds_and_forces_merges_where_it_blocks_them(n):
    v, ix = soup(n, n)
    free = P.build(v, ix, 1, 0, 8)
    assert free[2][7] <= P.nn_iterations(n)
    for extra in (0, 1, 3):
        D = P.clog2(n) + extra
        nodes, tris, info = P.build(v, ix, 1, 0, 8, depth_limit=D)
        assert info[1] == T.check_structure(nodes, tris, n, 1) <= D, (D, info[1])
        if extra == 0:                                     # no merge is admissible: I idle iterations, then clog2(n) forced ones
            assert info[7] == P.nn_iterations(n) + P.clog2(n)
            assert info[1] == P.clog2(n)
    same = P.build(v, ix, 1, 0, 8, depth_limit=56)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(free, same))
    assert free[2][1] < 56


def test_split_references_go_through_the_clustering(cornell_scene):
    for name, (v, ix), budget, pieces in (("cornell", (cornell_scene.vertices, cornell_scene.indices), 1.0, 64),
                                          ("soup", soup(257, 6), 2.0, 8)):
        for max_leaf, passes in ((2, 0), (4, 2)):
            st = {}
            SP.build(v, ix, max_leaf, passes, budget, pieces, stats=st)
            nodes, tris, info = P.build(v, ix, max_leaf, passes, 8, budget=budget, max_pieces=pieces)
            assert info[4] == len(tris) == st["refs"] > len(ix), name
            assert (info[5], info[6]) == (st["split"], st["unmade"])
            depth = SP.check_split_structure(nodes, tris, len(ix), max_leaf, pieces)
            assert (info[0], info[1]) == (len(nodes), depth)


def test_atrium_costs(tmp_path):
    """Conditions with a margin over what a numpy prototype of the rule gave on the atrium (264 884 triangles, max_leaf 2, default costs,
    root cost over the root's half area): LBVH 137.87, 3 treelet passes 82.97, PLOC radius 16 83.54 (0.606 x the LBVH), PLOC radius 16 +
    1 pass 76.98 (0.928 x the 3 passes), 63 iterations."""
    from rodent_amd import scenes
    sc = S.convert(scenes.scene_obj("atrium"), tmp_path / "atrium.rscene")
    codes, leafbox, _, _ = sorted_refs(sc.vertices, sc.indices)
    cost = {}
    with np.errstate(all="ignore"):
        for passes in (0, 3):
            t = T.Tree(*L.karras(codes), leafbox, 2, T.NODE_COST, T.TRI_COST)
            t.fit()
            for k in range(passes):
                t.treelet_pass(T.gamma(k))
            t.fit()
            cost["lbvh", passes] = P.root_cost(t)
    for passes in (0, 1):
        t, iterations = P.fitted(leafbox, 2, passes, 16)
        cost["ploc", passes] = P.root_cost(t)
        assert iterations <= P.nn_iterations(len(leafbox)), iterations
    print({k: round(c, 2) for k, c in cost.items()}, "iterations", iterations)
    assert cost["ploc", 0] <= 0.65 * cost["lbvh", 0]
    assert cost["ploc", 1] <= 0.96 * cost["lbvh", 3]
