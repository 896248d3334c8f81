"""The forest build (rodent_hip_build_objects, csrc/build_forest.h: k_bf_*; instances.build_objects / rebuild_objects) on the GPU.

The contract is byte equality with the per-object builder: for max_leaf 1, 2 and 8 the packed records, the table and the info words of
tests/forest_build_model.py's fixture objects equal the model (lbvh_model.build per object) and pack_objects of per-object
gpubuild.build_bvh2, in pack mode and in place, in any list order, on any stream, whatever the scratch held; flags stay inside their
object; a refused range has nothing touched; a slotted set traces like the packed per-object builds, before and after a rebuild; the
renderer's instanced scene, created through the one-list path, has the model's tables.
"""
import ctypes as C

import numpy as np
import pytest

import forest_build_model as FB
from rodent_amd import formats as F
from test_gpu_instanced_render import R, assert_tables, expected_tables, parts, rendering  # noqa: F401  (fixtures and the table check)

pytestmark = pytest.mark.gpu
MAX_LEAVES = (1, 2, 8)
PACK, IN_PLACE = 1, 0
BAD_INDEX, NON_FINITE, BAD_TOPOLOGY, BAD_OBJECT = 1, 2, 4, 8
FILL = 0xA5


@pytest.fixture(scope="module")
def mods(native_build):
    import torch
    from rodent_amd import abi, gpubuild, instances
    assert torch.cuda.is_available(), "these tests need a GPU"
    return abi, gpubuild, instances


class Forest:
    """The fixture objects' concatenated tables and, per max_leaf, the model: computed once, never changed."""

    def __init__(self, meshes, max_leaves=MAX_LEAVES):
        self.vertices, self.indices, self.ranges = FB.concat(meshes)
        self.model = {m: FB.build(self.vertices, self.indices, self.ranges, m) for m in max_leaves}
        self.alone = {m: FB.objects_of(*self.model[m][:3]) for m in max_leaves}
        self.slot_offset, self.room = FB.slots(self.ranges)

    def slotted_table(self):
        t = np.zeros(len(self.ranges), F.OBJECT)
        t["node_offset"], t["tri_offset"], t["num_tris"] = self.slot_offset, self.ranges[:, 0], self.ranges[:, 1]
        return t


@pytest.fixture(scope="module")
def forest():
    return Forest(FB.fixture_meshes())


@pytest.fixture(scope="module")
def many():
    return Forest(FB.many_meshes())


class Result:
    pass


def run(mods, fo, max_leaf, mode, listed=None, ranges=None, edit=None, vertices=None, stream=None, scratch_fill=None):
    """One rodent_hip_build_objects call on buffers pre-filled with 0xA5: the node buffer has the slotted room, the table uploaded is
    zeros in pack mode and the slotted table in place, `edit(ranges)` may change the planned range table.  Returns the host copies."""
    import torch
    abi, gb, gi = mods
    l = abi.lib()
    K = len(fo.ranges)
    listed = np.arange(K) if listed is None else np.asarray(listed)
    rows = fo.ranges[np.clip(listed, 0, K - 1)] if ranges is None else np.asarray(ranges, np.int32)
    ids, first, count = (np.ascontiguousarray(a, np.int32) for a in (listed, rows[:, 0], rows[:, 1]))
    rt, totals = np.zeros(len(ids), F.REFIT_RANGE), np.zeros(2, np.int32)
    need = l.rodent_hip_build_objects_plan(ids.ctypes.data, first.ctypes.data, count.ctypes.data, len(ids), rt.ctypes.data,
                                           totals.ctypes.data)
    assert need > 0
    if edit:
        edit(rt)
    table = np.zeros(K, F.OBJECT) if mode == PACK else fo.slotted_table()
    v = torch.from_numpy(np.ascontiguousarray(fo.vertices if vertices is None else vertices)).cuda()
    ix = torch.from_numpy(fo.indices).cuda()
    nodes = torch.full((int(fo.room.sum()) * F.NODE2.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    tris = torch.full((len(fo.indices) * F.TRI1.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    table_dev, rt_dev = abi.to_device(table, 0), abi.to_device(rt, 0)
    scratch = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    object_info = torch.full((len(ids), 4), 77, dtype=torch.int32, device="cuda")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = l.rodent_hip_build_objects(0, v.data_ptr(), len(v), ix.data_ptr(), len(ix), max_leaf, mode, nodes.data_ptr(), tris.data_ptr(),
                                    table_dev.data_ptr(), K, rt_dev.data_ptr(), len(ids), int(totals[0]), scratch.data_ptr(),
                                    object_info.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
    assert rc == 0
    stream.synchronize()
    r = Result()
    r.nodes, r.tris = nodes.cpu().numpy().view(F.NODE2), tris.cpu().numpy().view(F.TRI1)
    r.table, r.object_info, r.info = abi.from_device(table_dev, F.OBJECT), object_info.cpu().numpy(), info.cpu().numpy()
    return r


def filled(records):
    return (records.view(np.uint8) == FILL).all()


def object_bytes(r, k):
    t = r.table[k]
    return (r.nodes[t["node_offset"]: t["node_offset"] + t["num_nodes"]].tobytes(),
            r.tris[t["tri_offset"]: t["tri_offset"] + t["num_tris"]].tobytes())


def model_bytes(fo, max_leaf, k):
    return fo.alone[max_leaf][k][0].tobytes(), fo.alone[max_leaf][k][1].tobytes()


def assert_slots(r, fo, max_leaf, complete, untouched=()):
    """In place: every object of `complete` equals the model in its slot, the rest of every slot and everything of `untouched`
    objects still holds the fill."""
    for k in range(len(fo.ranges)):
        off, room, (first, n) = int(fo.slot_offset[k]), int(fo.room[k]), fo.ranges[k]
        slot, recs = r.nodes[off: off + room], r.tris[first: first + n]
        if k in complete:
            want = fo.alone[max_leaf][k]
            assert r.table[k]["num_nodes"] == len(want[0]), k
            assert slot[: len(want[0])].tobytes() == want[0].tobytes() and recs.tobytes() == want[1].tobytes(), k
            assert filled(slot[len(want[0]):]), k
        elif k in untouched:
            assert filled(slot) and filled(recs) and r.table[k]["num_nodes"] == 0, k


# ---- pack mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_pack_mode_equals_the_model_and_the_per_object_builds(mods, forest, max_leaf):
    abi, gb, gi = mods
    nodes, tris, table, info = forest.model[max_leaf]
    r = run(mods, forest, max_leaf, PACK)
    assert r.table.tobytes() == table.tobytes()
    assert r.nodes[: len(nodes)].tobytes() == nodes.tobytes() and r.tris.tobytes() == tris.tobytes()
    assert filled(r.nodes[len(nodes):])
    assert r.object_info.tolist() == info.tolist()
    assert r.info.tolist() == [len(nodes), int(info[:, 1].max()), 0, 0]
    # the per-object builder and pack_objects; the Python entry
    built = [gb.build_bvh2(forest.vertices, forest.indices[f: f + n], max_leaf) for f, n in forest.ranges]
    assert [b.info.tolist() for b in built] == r.object_info.tolist()
    packed = gi.pack_objects(built)
    objects = gi.build_objects(forest.vertices, forest.indices, forest.ranges, max_leaf)
    for o in (packed, objects):
        assert o.table.tobytes() == table.tobytes() and abi.from_device(o.table_dev, F.OBJECT).tobytes() == table.tobytes()
        assert o.nodes.cpu().numpy().tobytes() == nodes.tobytes() and o.tris.cpu().numpy().tobytes() == tris.tobytes()
    assert objects.depths.tolist() == info[:, 1].tolist() and objects.capacities is None and packed.capacities is None
    assert (objects.num_objects, objects.num_nodes, objects.num_tris) == (len(table), len(nodes), len(tris))


# ---- in place -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_in_place_fills_the_slots_and_nothing_else_in_any_list_order(mods, forest, max_leaf):
    K = len(forest.ranges)
    r = run(mods, forest, max_leaf, IN_PLACE)
    assert_slots(r, forest, max_leaf, complete=range(K))
    assert r.object_info.tolist() == forest.model[max_leaf][3].tolist()
    order = np.array([5, 2, 7, 0, 6, 4, 1, 3])
    p = run(mods, forest, max_leaf, IN_PLACE, listed=order)
    assert p.nodes.tobytes() == r.nodes.tobytes() and p.tris.tobytes() == r.tris.tobytes() and p.table.tobytes() == r.table.tobytes()
    assert p.object_info.tolist() == r.object_info[order].tolist() and p.info.tolist() == r.info.tolist()
    # a subset: the unlisted objects' slots and table entries keep their bytes
    sub = run(mods, forest, max_leaf, IN_PLACE, listed=[FB.BIG, FB.PAIR, FB.EQUAL40])
    assert_slots(sub, forest, max_leaf, complete=(FB.BIG, FB.PAIR, FB.EQUAL40),
                 untouched=[k for k in range(K) if k not in (FB.BIG, FB.PAIR, FB.EQUAL40)])


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_rebuild_of_two_objects_after_their_vertices_moved(mods, forest, max_leaf):
    abi, gb, gi = mods
    objects = gi.build_objects(forest.vertices, forest.indices, forest.ranges, max_leaf, slots=True)
    assert objects.capacities.tolist() == forest.room.tolist() and objects.table["node_offset"].tolist() == forest.slot_offset.tolist()
    assert objects.table["num_nodes"].tolist() == forest.model[max_leaf][2]["num_nodes"].tolist()
    before = (objects.nodes.cpu().numpy().copy(), objects.tris.cpu().numpy().copy())
    listed = [FB.FLAT, FB.SINGLE]                                # objects [2, 0]
    moved = forest.vertices.copy()
    rng = np.random.default_rng(9)
    moved[:, :3] = (moved[:, :3] * np.float32(1.25) + rng.normal(0, 0.4, moved[:, :3].shape)).astype(np.float32)
    words, per_object = gi.rebuild_objects(objects, listed, moved, forest.indices, forest.ranges[listed], max_leaf)
    fresh = FB.build(moved, forest.indices, forest.ranges, max_leaf)
    alone = FB.objects_of(*fresh[:3])
    assert per_object.tolist() == fresh[3][listed].tolist() and words[2] == 0
    nodes, tris = objects.nodes.cpu().numpy(), objects.tris.cpu().numpy()
    for k in range(len(forest.ranges)):
        off, room, (first, n) = int(forest.slot_offset[k]), int(forest.room[k]), forest.ranges[k]
        node_bytes = slice(off * F.NODE2.itemsize, (off + room) * F.NODE2.itemsize)
        tri_bytes = slice(first * F.TRI1.itemsize, (first + n) * F.TRI1.itemsize)
        if k in listed:
            built = gb.download(gb.build_bvh2(moved, forest.indices[first: first + n], max_leaf))
            for want in (alone[k], built):
                assert nodes[node_bytes][: want[0].nbytes].tobytes() == want[0].tobytes() and tris[tri_bytes].tobytes() == want[1].tobytes()
            assert objects.table[k]["num_nodes"] == len(alone[k][0]) and objects.depths[k] == fresh[3][k][1]
        else:
            assert nodes[node_bytes].tobytes() == before[0][node_bytes].tobytes(), k
            assert tris[tri_bytes].tobytes() == before[1][tri_bytes].tobytes(), k
    tight = gi.build_objects(forest.vertices, forest.indices, forest.ranges, max_leaf)
    with pytest.raises(ValueError):
        gi.rebuild_objects(tight, listed, moved, forest.indices, forest.ranges[listed], max_leaf)
    with pytest.raises(ValueError):
        gi.rebuild_objects(objects, [FB.PAIR], moved, forest.indices, [(1, 1)], max_leaf)


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_two_streams_and_dirty_scratch_give_the_same_bytes(mods, forest, max_leaf):
    import torch
    a = run(mods, forest, max_leaf, PACK, stream=torch.cuda.Stream(), scratch_fill=0xFF)
    b = run(mods, forest, max_leaf, PACK, stream=torch.cuda.Stream(), scratch_fill=0xFF)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.tris.tobytes() == b.tris.tobytes() and a.table.tobytes() == b.table.tobytes()
    assert a.object_info.tolist() == b.object_info.tolist() == forest.model[max_leaf][3].tolist()
    assert a.nodes[: len(forest.model[max_leaf][0])].tobytes() == forest.model[max_leaf][0].tobytes()


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_three_hundred_objects_in_both_modes(mods, many, max_leaf):
    nodes, tris, table, info = many.model[max_leaf]
    r = run(mods, many, max_leaf, PACK, scratch_fill=0xFF)
    assert r.table.tobytes() == table.tobytes() and r.object_info.tolist() == info.tolist()
    assert r.nodes[: len(nodes)].tobytes() == nodes.tobytes() and r.tris.tobytes() == tris.tobytes() and filled(r.nodes[len(nodes):])
    order = np.random.default_rng(4).permutation(len(many.ranges))
    p = run(mods, many, max_leaf, IN_PLACE, listed=order, scratch_fill=0xFF)
    assert_slots(p, many, max_leaf, complete=range(len(many.ranges)))
    assert p.object_info.tolist() == info[order].tolist() and p.info.tolist() == r.info.tolist()


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
@pytest.mark.parametrize("mode", (PACK, IN_PLACE))
def test_input_flags_stay_inside_their_objects(mods, forest, max_leaf, mode):
    K = len(forest.ranges)
    broken = Forest.__new__(Forest)
    broken.__dict__.update(forest.__dict__)
    broken.indices = forest.indices.copy()
    broken.indices[forest.ranges[FB.SOUP67][0] + 5, 1] = len(forest.vertices) + 3            # a vertex index outside the table
    vertices = forest.vertices.copy()
    vertices[forest.indices[forest.ranges[FB.FLAT_AXIS][0] + 7, 2], 1] = np.nan              # a NaN in another object
    r = run(mods, broken, max_leaf, mode, vertices=vertices)
    want = np.zeros(K, np.int32); want[FB.SOUP67], want[FB.FLAT_AXIS] = BAD_INDEX, NON_FINITE
    assert r.object_info[:, 2].tolist() == want.tolist() and r.info[2] == BAD_INDEX | NON_FINITE
    sound = [k for k in range(K) if not want[k]]
    assert (r.object_info[sound] == forest.model[max_leaf][3][sound]).all()
    for k in sound:
        assert object_bytes(r, k) == model_bytes(forest, max_leaf, k), k
    # the flagged objects are what the per-object builder makes of the same input
    fresh = FB.build(vertices, broken.indices, forest.ranges, max_leaf)
    for k in (FB.SOUP67, FB.FLAT_AXIS):
        mine = FB.objects_of(*fresh[:3])[k]
        assert object_bytes(r, k) == (mine[0].tobytes(), mine[1].tobytes()) and r.object_info[k].tolist() == fresh[3][k].tolist()


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_refused_ranges_have_nothing_touched(mods, forest, max_leaf):
    abi, gb, gi = mods
    K, last = len(forest.ranges), FB.SOUP_SCALED
    others = [k for k in range(K) if k != last]

    def check(r, flag, refused=last):
        assert r.object_info[refused].tolist() == [0, 0, flag, 0] and r.info[2] == flag
        assert r.object_info[[k for k in range(K) if k != refused], 2].tolist() == [0] * (K - 1)
        assert_slots(r, forest, max_leaf, complete=[k for k in range(K) if k != refused], untouched=[refused])
    # an object id outside the table, behind it and negative: nothing of the range's triangles is built anywhere
    for bad in (K, -1):
        listed = np.arange(K); listed[last] = bad
        r = run(mods, forest, max_leaf, IN_PLACE, listed=listed, ranges=forest.ranges)
        check(r, BAD_OBJECT)
    # rows beyond the index table
    def beyond_rows(rt): rt["first_tri"][last] = len(forest.indices) - forest.ranges[last][1] + 1
    check(run(mods, forest, max_leaf, IN_PLACE, edit=beyond_rows), BAD_TOPOLOGY)
    # a stretch beyond the totals (the position it gives up falls to the range in front, which ignores it)
    def beyond_totals(rt): rt["rec_start"][last] += 1; rt["node_start"][last] += 1
    check(run(mods, forest, max_leaf, IN_PLACE, edit=beyond_totals), BAD_TOPOLOGY)
    # in place, a triangle count that is not the table's
    rows = forest.ranges.copy(); rows[FB.PAIR, 1] = 1
    r = run(mods, forest, max_leaf, IN_PLACE, ranges=rows)
    check(r, BAD_TOPOLOGY, refused=FB.PAIR)
    # ... which pack mode accepts: the object is then its first triangle alone
    r = run(mods, forest, max_leaf, PACK, ranges=rows)
    assert r.info[2] == 0 and list(r.table[FB.PAIR].tolist()[2:]) == [1, 1]
    # the Python entries name the first flagged object
    objects = gi.build_objects(forest.vertices, forest.indices, forest.ranges, max_leaf, slots=True)
    vertices = forest.vertices.copy(); vertices[forest.indices[forest.ranges[FB.FLAT][0], 0], 0] = np.inf
    with pytest.raises(gb.BuildError, match=f"object {FB.FLAT}: non-finite"):
        gi.rebuild_objects(objects, [FB.SINGLE, FB.FLAT], vertices, forest.indices, forest.ranges[[FB.SINGLE, FB.FLAT]], max_leaf)
    with pytest.raises(gb.BuildError, match="object 9: object index"):
        gi.rebuild_objects(objects, [FB.SINGLE, 9], forest.vertices, forest.indices, forest.ranges[[FB.SINGLE, FB.FLAT]], max_leaf)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def cornell_mesh(cornell):
    """The Cornell box's triangles, from the committed BVH's Tri1 records in prim-id order."""
    t = cornell.blocks[2][1]
    t = t[np.argsort(t["prim_id"] & 0x7FFFFFFF, kind="stable")]
    corners = np.stack([t["v0"], t["v0"] - t["e1"], t["v0"] + t["e2"]], 1).astype(np.float32)
    return corners.reshape(-1, 3), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("max_leaf", MAX_LEAVES)
def test_a_slotted_set_traces_like_the_packed_per_object_builds(mods, cornell, max_leaf):
    abi, gb, gi = mods
    meshes = FB.fixture_meshes()
    fo = Forest([cornell_mesh(cornell), meshes[FB.SOUP67], meshes[FB.EQUAL40], meshes[FB.FLAT]], max_leaves=())
    place = lambda s, t: np.float32([s[0], 0, 0, t[0], 0, s[1], 0, t[1], 0, 0, s[2], t[2]])
    # the box under the identity; the others between the camera (0, 1, 2.7, looking down -z) and the box's own contents
    transforms = np.stack([place((1, 1, 1), (0, 0, 0)), place((0.04, 0.04, 0.04), (0, 1.0, 0.8)),
                           place((0.03, -0.05, 0.04), (-0.5, 0.6, 0.7)),
                           place((0.3, 0.3, 0.3), (0.4, 0.5, 0.8)), place((0.2, 0.4, -0.2), (-0.3, 1.4, 0.9)),
                           place((0.25, 0.25, 1), (0.3, 1.5, 0.2))])
    ids = np.int32([0, 1, 1, 2, 2, 3])
    rays = cornell.ray_sets["primary"]
    assert len(rays) == 64 * 64

    def both(vertices, slotted):
        packed = gi.pack_objects([gb.build_bvh2(vertices, fo.indices[f: f + n], max_leaf) for f, n in fo.ranges])
        out = []
        for objects in (packed, slotted):
            tlas = gi.build_tlas(objects, transforms, ids)
            out.append(gi.trace(objects, tlas, rays))
        (h0, i0), (h1, i1) = out
        assert h0.tobytes() == h1.tobytes() and i0.tolist() == i1.tolist()
        return h0, i0
    slotted = gi.build_objects(fo.vertices, fo.indices, fo.ranges, max_leaf, slots=True)
    hits, inst = both(fo.vertices, slotted)
    assert set(inst.tolist()) >= {0, 1} and len(set(inst.tolist()) - {-1, 0}) >= 2     # the box and copies of other objects are seen
    moved = fo.vertices.copy()
    f, n = fo.ranges[1]
    used = np.unique(fo.indices[f: f + n, :3])
    moved[used, :3] = (moved[used, :3] * np.float32([1.5, 0.5, 1.0]) + np.float32([2, 0, -3])).astype(np.float32)
    gi.rebuild_objects(slotted, [1], moved, fo.indices, fo.ranges[[1]], max_leaf)
    hits2, inst2 = both(moved, slotted)
    assert hits2.tobytes() != hits.tobytes()


# ---- scene creation ---------------------------------------------------------------------------------------------------------------------
def test_scene_creation_through_the_one_list_path_has_the_models_tables(R, parts):
    with rendering(R, parts, build=None) as r:
        nodes, tris = r.scene_bvh()
        assert nodes.tobytes() == parts.hierarchy[0].tobytes() and tris.tobytes() == parts.hierarchy[1].tobytes()
        assert_tables(r.instance_tables(), expected_tables(parts, parts.transforms), "created by one launch list")
