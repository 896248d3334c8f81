"""tests/refit_wide_model.py (the CPU model of rodent_hip_refit_bvh4_tri4 / _bvh8_tri4) against the rules of include/rodent_build.h.

On the BVH4 / BVH8 blocks of tests/golden/cornell.bvh with the Cornell mesh of the converter, and on hand-made trees:
* after a deformation every slot box is exactly the union of the triangle boxes under it (computed top-down here, not by the model's
  climb) and holds every corner of every triangle under it;
* refitted with its own vertices the host tree keeps its Tri4 bytes, and every refitted box contains the stored one;
* invalid lanes and the prim_id / geom_id / child / pad words are never touched;
* malformed trees raise RODENT_BUILD_BAD_TOPOLOGY with the predicted count of completed nodes.
The hand-made trees and their meshes are also what tests/test_gpu_refit_wide.py runs on the device.
"""
import numpy as np
import pytest

import refit_wide_model as W
import wide_fixtures as X
from conftest import GOLDEN
from lbvh_model import boxes_of, load_triangles
from rodent_amd import formats as F
from rodent_amd import scene as S

WIDTHS = (4, 8)
NODE = {4: F.NODE4, 8: F.NODE8}
INT_MIN = np.int32(-2 ** 31)
JUNK = np.float32(7.25)                # what the hand-made trees keep in their invalid lanes: a refit must leave it there


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


# ---- hand-made trees ---------------------------------------------------------------------------------------------------------

def empty_nodes(width, count):
    nodes = np.zeros(count, NODE[width])
    nodes["bounds"][:, 0::2, :] = np.inf
    nodes["bounds"][:, 1::2, :] = -np.inf
    return nodes


def packets(*ids):
    """Tri4 packets with these prim_id rows; geometry words hold JUNK, to be replaced in the valid lanes only."""
    tris = np.zeros(len(ids), F.TRI4)
    for name in ("v0", "e1", "e2", "n"):
        tris[name] = JUNK
    tris["prim_id"] = np.int32(ids)
    tris["geom_id"] = 3
    return tris


def strip_mesh(n):
    """n triangles along x over 3n vertices, none degenerate, no two alike."""
    v = np.zeros((3 * n, 4), np.float32)
    for t in range(n):
        v[3 * t: 3 * t + 3, :3] = np.float32([[2 * t, 0, 0.5 * t], [2 * t + 1, 0.25, t], [2 * t, 1, 1 - t]])
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


def one_leaf_tree(width):
    """One node, one leaf, one triangle."""
    nodes = empty_nodes(width, 1)
    nodes["child"][0, 0] = ~0
    return nodes, packets([0, -1, -1, INT_MIN]), *strip_mesh(1)


def nine_triangle_leaf_tree(width):
    """One node: a leaf of 9 triangles in packets of 4, 4 and 1 -- lane 3 of the first two is valid and carries no end bit -- and a
    leaf whose only packet has a hole: [9, 10, -1, INT_MIN | 5], lanes 2 and 3 are not valid."""
    nodes = empty_nodes(width, 1)
    nodes["child"][0, :2] = [~0, ~3]
    tris = packets([0, 1, 2, 3], [4, 5, 6, 7], [8, -1, -1, -1], [9, 10, -1, INT_MIN | np.int32(5)])
    return nodes, tris, *strip_mesh(11)


def three_node_tree(width):
    """Root 0 with inner slots 0 and 1 (nodes 1 and 2) and a leaf; node 1: two leaves; node 2: one leaf of two packets.
    7 packets, 12 triangles, the last packet ends the last leaf."""
    nodes = empty_nodes(width, 3)
    nodes["child"][0, :3] = [2, 3, ~0]
    nodes["child"][1, :2] = [~1, ~2]
    nodes["child"][2, 1] = ~5                                     # slot 0 of node 2 is empty: not packed from the front
    tris = packets([0, -1, -1, INT_MIN], [1, 2, -1, -1], [3, 4, 5, 6], [7, 8, 9, INT_MIN | np.int32(10)], [0, 0, 0, 0],
                   [11, 3, 7, 1], [2, -1, -1, -1])
    tris["prim_id"][4] = [5, -1, -1, -1]                          # a leaf nobody names, between the others
    return nodes, tris, *strip_mesh(12)


def mesh_of(tris):
    """The mesh a hand-made Tri4 array was made from: triangle t = prim id, corners v0, v0 - e1, v0 + e2 over vertices 3t ... 3t + 2."""
    flat, ids = X.flatten_tri4(tris)
    n = int(ids.max()) + 1
    v = np.zeros((3 * n, 4), np.float32)
    v[3 * ids, :3], v[3 * ids + 1, :3], v[3 * ids + 2, :3] = flat["v0"], flat["v0"] - flat["e1"], flat["v0"] + flat["e2"]
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    return v, ix


def chain_tree(width, depth=40):
    nodes, tris = X.chain_wide(width, depth, fan=width - 1)
    return nodes, tris, *mesh_of(tris)


HAND_MADE = {"one_leaf": one_leaf_tree, "nine": nine_triangle_leaf_tree, "three_nodes": three_node_tree, "chain40": chain_tree}


# ---- the rules, stated top-down ----------------------------------------------------------------------------------------------

def leaf_triangles(tris, first):
    out, p = [], first
    while True:
        ids = tris["prim_id"][p]
        for k in range(4):
            if ids[k] == -1:
                break
            out.append(int(ids[k]) & 0x7FFFFFFF)
        if ids[3] < 0:
            return out
        p += 1


def slots(nodes, tris, i=0):
    """Yields (node, slot, ids of the triangles under that slot) for every slot with a child below node i, a node's own slots last."""
    for k, c in enumerate(nodes["child"][i]):
        if c < 0:
            yield i, k, leaf_triangles(tris, ~int(c))
        elif c > 0:
            ids = []
            for entry in slots(nodes, tris, int(c) - 1):
                if entry[0] == int(c) - 1:
                    ids += entry[2]
                yield entry
            yield i, k, ids


def assert_exact_and_covering(nodes, tris, vertices, indices):
    """Every slot box is the union of the triangle boxes under it, bit for bit, and holds their corners; returns the slots seen."""
    V, _, _ = load_triangles(vertices, indices)
    tbox = boxes_of(V + np.float32(0))
    count = 0
    for i, k, ids in slots(nodes, tris):
        b = tbox[ids]
        want = np.empty(6, np.float32)
        want[0::2], want[1::2] = b[:, 0::2].min(0), b[:, 1::2].max(0)
        got = nodes["bounds"][i][:, k]
        assert got.tobytes() == want.tobytes(), (i, k)
        corners = V[ids].reshape(-1, 3)
        assert (corners >= got[0::2]).all() and (corners <= got[1::2]).all(), (i, k)
        count += 1
    return count


def assert_columns_are_the_triangles(tris, vertices, indices):
    """Every valid lane holds v0, e1 = v0 - v1, e2 = v2 - v0 of its triangle and n = e1 x e2 with every product rounded to fp32."""
    valid = W.valid_lanes(tris)
    V, _, _ = load_triangles(vertices, indices[tris["prim_id"][valid] & 0x7FFFFFFF])
    v0, e1, e2 = V[:, 0], V[:, 0] - V[:, 1], V[:, 2] - V[:, 0]
    x, y, z = 0, 1, 2
    n = np.stack([e1[:, y] * e2[:, z] - e1[:, z] * e2[:, y], e1[:, z] * e2[:, x] - e1[:, x] * e2[:, z],
                  e1[:, x] * e2[:, y] - e1[:, y] * e2[:, x]], 1)
    assert n.dtype == np.float32
    assert np.allclose(n, np.cross(e1.astype(np.float64), e2.astype(np.float64)), rtol=1e-4, atol=1e-4)
    for name, want in (("v0", v0), ("e1", e1), ("e2", e2), ("n", n)):
        assert tris[name].transpose(0, 2, 1)[valid].tobytes() == want.tobytes(), name


def assert_only_the_rules_words_change(before, after):
    """(nodes, tris) pairs: child, pad, prim_id, geom_id and every invalid lane keep their bytes."""
    for name in ("child", "pad"):
        assert before[0][name].tobytes() == after[0][name].tobytes(), name
    for name in ("prim_id", "geom_id"):
        assert before[1][name].tobytes() == after[1][name].tobytes(), name
    invalid = ~W.valid_lanes(before[1])
    for name in ("v0", "e1", "e2", "n"):
        a, b = before[1][name].transpose(0, 2, 1)[invalid], after[1][name].transpose(0, 2, 1)[invalid]
        assert a.tobytes() == b.tobytes(), name


# ---- tests -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", WIDTHS)
def test_cornell_after_a_deformation_is_exact_and_covering(cornell, cornell_scene, width):
    nodes, tris = cornell.blocks[width]
    v, ix = cornell_scene.vertices, cornell_scene.indices
    moved = W.deform(v, ix, seed=width)
    out_nodes, out_tris, info = W.refit(width, nodes, tris, moved, ix)
    lanes = int(W.valid_lanes(tris).sum())
    assert info.tolist() == [len(nodes), lanes, 0, 0] and lanes >= len(ix)
    assert assert_exact_and_covering(out_nodes, out_tris, moved, ix) == int((nodes["child"] != 0).sum())
    assert out_nodes.tobytes() != nodes.tobytes() and out_tris.tobytes() != tris.tobytes()
    assert_only_the_rules_words_change((nodes, tris), (out_nodes, out_tris))
    assert_columns_are_the_triangles(out_tris, moved, ix)


@pytest.mark.parametrize("width", WIDTHS)
def test_cornell_with_its_own_vertices_keeps_its_tri4_bytes_and_its_boxes_only_grow(cornell, cornell_scene, width):
    nodes, tris = cornell.blocks[width]
    out_nodes, out_tris, info = W.refit(width, nodes, tris, cornell_scene.vertices, cornell_scene.indices)
    assert info.tolist() == [len(nodes), int(W.valid_lanes(tris).sum()), 0, 0]
    for name in ("v0", "e1", "e2", "n"):                       # n too: the host builder's cross rounds each product, as the rules do
        assert out_tris[name].tobytes() == tris[name].tobytes(), name
    assert out_tris.tobytes() == tris.tobytes()
    assert W.contains(out_nodes, nodes).all()
    assert_only_the_rules_words_change((nodes, tris), (out_nodes, out_tris))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_trees(width, name):
    nodes, tris, v, ix = HAND_MADE[name](width)
    moved = W.deform(v, ix, seed=5, collapse=1)
    out_nodes, out_tris, info = W.refit(width, nodes, tris, moved, ix)
    lanes = int(W.valid_lanes(tris).sum())
    assert info.tolist() == [len(nodes), lanes, 0, 0]
    assert lanes == {"one_leaf": 1, "nine": 11, "three_nodes": 17, "chain40": 40 * (width - 1) + 1}[name]
    assert assert_exact_and_covering(out_nodes, out_tris, moved, ix) == int((nodes["child"] != 0).sum())
    assert_only_the_rules_words_change((nodes, tris), (out_nodes, out_tris))
    empty = nodes["child"] == 0                                  # empty slots keep their stored bounds
    assert out_nodes["bounds"].transpose(0, 2, 1)[empty].tobytes() == nodes["bounds"].transpose(0, 2, 1)[empty].tobytes()
    assert_columns_are_the_triangles(out_tris, moved, ix)


def malformed(width):
    """name -> (nodes, tris, vertices, indices, predicted info) on the three-node tree: [nodes completed, lanes, flags, 0]."""
    nodes, tris, v, ix = three_node_tree(width)
    cases = {}
    a = nodes.copy(); a["child"][1, 3] = len(nodes) + 5          # node 1 waits for a child that is not there; the root waits for node 1
    cases["child out of range"] = (a, tris, v, ix, [1, 17, W.BAD_TOPOLOGY, 0])
    a = nodes.copy(); a["child"][0, 3] = 2                       # the root names node 1 twice: one arrival short
    cases["node claimed twice"] = (a, tris, v, ix, [2, 17, W.BAD_TOPOLOGY, 0])
    a = nodes.copy(); a["child"][0, 3] = 1                       # the root as a child
    cases["root as a child"] = (a, tris, v, ix, [2, 17, W.BAD_TOPOLOGY, 0])
    t = tris.copy(); t["prim_id"][6, 3] = 6                      # the last leaf never ends: its slot stays, its node still completes
    cases["leaf without end"] = (nodes, t, v, ix, [3, 17, W.BAD_TOPOLOGY, 0])
    a = nodes.copy(); a["child"][2, 2] = ~len(tris)
    cases["leaf start beyond the packets"] = (a, tris, v, ix, [3, 17, W.BAD_TOPOLOGY, 0])
    t = tris.copy(); t["prim_id"][3, 3] = INT_MIN | np.int32(len(ix))
    cases["prim id beyond the table"] = (nodes, t, v, ix, [3, 16, W.BAD_TOPOLOGY, 0])
    return cases


@pytest.mark.parametrize("width", WIDTHS)
def test_malformed_trees_raise_the_flag_with_the_predicted_count(width):
    sound = three_node_tree(width)
    for name, (nodes, tris, v, ix, want) in malformed(width).items():
        out_nodes, out_tris, info = W.refit(width, nodes, tris, v, ix)
        assert info.tolist() == want, name
        assert_only_the_rules_words_change((nodes, tris), (out_nodes, out_tris))
        if name == "child out of range":                         # the flagged slot stays as stored
            assert out_nodes["bounds"][1][:, 3].tobytes() == nodes["bounds"][1][:, 3].tobytes()
        if name == "leaf without end":
            assert out_nodes["bounds"][2][:, 1].tobytes() == nodes["bounds"][2][:, 1].tobytes()
        if name == "prim id beyond the table":                   # that lane stays, the others of its packet are rewritten
            assert (out_tris["v0"][3][:, 3] == JUNK).all() and (out_tris["v0"][3][:, :3] != JUNK).any()
            good = W.refit(width, *sound)[0]
            assert W.contains(good, out_nodes).all() and good.tobytes() != out_nodes.tobytes()
    bad = sound[3].copy(); bad[5, 1] = len(sound[2])
    assert W.refit(width, sound[0], sound[1], sound[2], bad)[2].tolist() == [3, 17, 1, 0]
    nan = sound[2].copy(); nan[4, 1] = np.nan
    assert W.refit(width, sound[0], sound[1], nan, sound[3])[2].tolist() == [3, 17, 2, 0]
