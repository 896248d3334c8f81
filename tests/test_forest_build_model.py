"""The fixtures of the forest build's tests are not vacuous (tests/forest_build_model.py): three perturbed models -- equal codes told
apart by global sorted positions, one frame for all objects, a Karras search bounded by the total instead of the object -- each differ
from the true model in at least one object's bytes, and the true model's tight packing has instances.pack_objects' offsets."""
import numpy as np
import pytest

import forest_build_model as FB
import lbvh_model as L


@pytest.fixture(scope="module")
def forest():
    v, ix, ranges = FB.concat(FB.fixture_meshes())
    return v, ix, ranges, FB.build(v, ix, ranges, 2)


def differing(a, b):
    """The objects whose bytes differ between two packed results."""
    pa, pb = FB.objects_of(*a[:3]), FB.objects_of(*b[:3])
    return [k for k, (x, y) in enumerate(zip(pa, pb)) if x[0].tobytes() != y[0].tobytes() or x[1].tobytes() != y[1].tobytes()]


def test_tight_packing_has_pack_objects_offsets(forest):
    v, ix, ranges, (nodes, tris, table, info) = forest
    assert table["num_tris"].tolist() == ranges[:, 1].tolist() and table["tri_offset"].tolist() == ranges[:, 0].tolist()
    assert table["node_offset"].tolist() == (np.cumsum(table["num_nodes"]) - table["num_nodes"]).tolist()
    assert len(nodes) == table["num_nodes"].sum() and len(tris) == len(ix) and (info[:, 2] == 0).all()
    assert (info[:, 0] == table["num_nodes"]).all()
    for k, (f, n) in enumerate(ranges):
        alone = L.build(v, ix[f: f + n], 2)
        got = FB.objects_of(nodes, tris, table)[k]
        assert got[0].tobytes() == alone[0].tobytes() and got[1].tobytes() == alone[1].tobytes()
        assert (got[1]["prim_id"] & 0x7FFFFFFF).max() == n - 1                       # prim ids are object-local rows
    offsets, room = FB.slots(ranges)
    assert (room >= table["num_nodes"]).all() and offsets.tolist() == (np.cumsum(room) - room).tolist()


def test_global_tie_breaks_show(forest):
    v, ix, ranges, true = forest
    for max_leaf in (1, 2, 8):
        bad = differing(FB.build(v, ix, ranges, max_leaf), FB.build_global_ties(v, ix, ranges, max_leaf))
        assert FB.EQUAL40 in bad, max_leaf
    # an object that starts at a multiple of its size's power of two hides the mistake: the first object never differs
    assert FB.SINGLE not in bad and FB.PAIR not in bad


def test_a_shared_frame_shows(forest):
    v, ix, ranges, true = forest
    bad = differing(true, FB.build_shared_frame(v, ix, ranges, 2))
    assert FB.SOUP67 in bad and FB.BIG in bad


def test_an_unbounded_karras_search_shows(forest):
    v, ix, ranges, true = forest
    leaked, bounded = FB.karras_unbounded(v, ix, ranges)
    differs = [k for k, (a, b) in enumerate(zip(leaked, bounded))
               if a is not None and any(x.tolist() != y.tolist() for x, y in zip(a, b))]
    assert differs, "no object's Karras ranges change when the search may read the neighbouring object's codes"
    n = ranges[:, 1]
    assert any((leaked[k][1] >= n[k]).any() or (leaked[k][0] < 0).any() for k in differs)     # a range that leaves its object


def test_the_many_object_set_needs_a_second_rank_digit():
    v, ix, ranges = FB.concat(FB.many_meshes())
    assert len(ranges) > 256 and set(ranges[:, 1].tolist()) == {1, 2, 3}
    nodes, tris, table, info = FB.build(v, ix, ranges, 2)
    assert len(tris) == len(ix) and (info[:, 2] == 0).all()
