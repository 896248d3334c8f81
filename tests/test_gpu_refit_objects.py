"""The refit of listed objects of a packed set (rodent_hip_refit_objects, csrc/build_refit.h: k_forest_*; instances.refit_objects) on
the GPU, through the standalone ABI.

Four objects packed by pack_objects: one triangle (a single root with an empty slot), instance_model.flat_object, a 67-triangle
indexed soup at max_leaf 1 (66 nodes: the waves of the node space straddle objects) and a 1000-triangle soup built with treelet
passes.  Three of them are listed, not in ascending order, the unlisted one between two listed ones:

* every listed object equals refit_model.refit and gpubuild.refit_bvh2 of that object alone, byte for byte; the unlisted object keeps
  its bytes; the info words are exact; the list's order does not matter;
* refitted with the vertices they were built from, all objects keep every byte;
* a listed id outside the table raises RODENT_TLAS_BAD_OBJECT and the others come out complete; a corrupted child id raises
  RODENT_BUILD_BAD_TOPOLOGY in its object alone; a range whose stretch leaves the totals is flagged and has nothing touched; invalid
  arguments are refused on the host and enqueue nothing.  These are guard paths with defined results.
"""
import ctypes as C

import numpy as np
import pytest

import instance_model as IM
import refit_model as R
import scene_update_model as SU
from rodent_amd import formats as F
from test_gpu_build import soup

pytestmark = pytest.mark.gpu
SINGLE, FLAT, SOUP67, SOUP1000 = range(4)
LISTS = ((SOUP67, SOUP1000, SINGLE), (SINGLE, SOUP1000, FLAT))         # unlisted: FLAT between SINGLE and SOUP67 / SOUP67


@pytest.fixture(scope="module")
def mods(native_build):
    import torch
    from rodent_amd import abi, gpubuild, instances
    assert torch.cuda.is_available(), "these tests need a GPU"
    return abi, gpubuild, instances


@pytest.fixture(scope="module")
def forest(mods):
    """The four objects: per object (nodes, tris) as built, the concatenated vertex and index tables, the (first_tri, num_tris) rows,
    the moved vertices and, per object, the model's refit of it alone."""
    abi, gb, gi = mods
    z = 0.5
    meshes = [(np.float32([[0, 0, 0, 0], [1, 0, 0.5, 0], [0, 1, 1, 0]]), np.int32([[0, 1, 2, 0]])),
              (np.float32([[-1, -1, z, 0], [1, -1, z, 0], [1, 1, z, 0], [-1, 1, z, 0]]), np.int32([[0, 1, 2, 0], [0, 2, 3, 0]])),
              SU.indexed_soup(67, 68)[:2], soup(1000, 1002)]
    pairs = []
    for k, (v, ix) in enumerate(meshes):
        if k == FLAT:
            pairs.append(IM.flat_object(z))
        else:
            pairs.append(gb.download(gb.build_bvh2(v, ix, 1 if k == SOUP67 else 2, treelet_passes=3 if k == SOUP1000 else 0)))
    assert pairs[SINGLE][0]["child"].tolist() == [[~0, 0]] and len(pairs[SOUP67][0]) == 66
    vertices, indices, rows, base = [], [], [], 0
    for v, ix in meshes:
        ix = np.array(ix, np.int32)
        ix[:, :3] += base
        rows.append((sum(len(i) for i in indices), len(ix)))
        vertices.append(np.asarray(v, np.float32)); indices.append(ix)
        base += len(v)
    vertices, indices = np.concatenate(vertices), np.concatenate(indices)
    moved = R.deform(vertices, indices, seed=5)
    alone = [R.refit(*pairs[k], moved, indices[f: f + n]) for k, (f, n) in enumerate(rows)]
    assert all(m[2].tolist() == [len(p[0]), len(p[1]), 0, 0] for m, p in zip(alone, pairs))
    return dict(pairs=pairs, vertices=vertices, indices=indices, rows=np.int32(rows), moved=moved, alone=alone)


def download(objects):
    """[(nodes, tris)] per object of an ObjectSet."""
    nodes = objects.nodes.cpu().numpy().view(F.NODE2)
    tris = objects.tris.cpu().numpy().view(F.TRI1)
    return [(nodes[r["node_offset"]: r["node_offset"] + r["num_nodes"]].copy(), tris[r["tri_offset"]: r["tri_offset"] + r["num_tris"]].copy())
            for r in objects.table]


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("listed", LISTS)
def test_listed_objects_equal_the_model_and_the_single_refit(mods, forest, listed):
    abi, gb, gi = mods
    objects = gi.pack_objects(forest["pairs"])
    words = gi.refit_objects(objects, listed, forest["moved"], forest["indices"], forest["rows"][list(listed)])
    got = download(objects)
    total = [sum(len(forest["pairs"][k][j]) for k in listed) for j in (0, 1)]
    assert words.tolist() == [total[0], total[1], 0, 0]
    for k in range(4):
        if k in listed:
            assert same(got[k], forest["alone"][k]), k
            assert not same(got[k], forest["pairs"][k]), k
            f, n = forest["rows"][k]
            bvh = gb.refit_bvh2(abi.DeviceBvh(2, *forest["pairs"][k], 0), forest["moved"], forest["indices"][f: f + n])
            assert same(got[k], gb.download(bvh)), k
        else:
            assert same(got[k], forest["pairs"][k]), k
    # any order of the list, a prepared plan, another stream and a reused scratch: the same bytes
    import torch
    again = gi.pack_objects(forest["pairs"])
    order = listed[::-1]
    plan = gi.plan_refit(again, order, forest["rows"][list(order)])
    assert plan.num_listed == 3 and (plan.num_nodes, plan.num_recs) == tuple(total)
    assert plan.table["node_start"].tolist() == [0] + np.cumsum([len(forest["pairs"][k][0]) for k in order])[:-1].tolist()
    scratch = torch.empty(plan.scratch_bytes + 4096, dtype=torch.uint8, device="cuda").fill_(0xAB)
    moved_dev = torch.from_numpy(forest["moved"]).cuda()
    words = gi.refit_objects(again, None, moved_dev, forest["indices"], plan, stream=torch.cuda.Stream(), scratch=scratch)
    assert words.tolist() == [total[0], total[1], 0, 0]
    assert all(same(a, b) for a, b in zip(download(again), got))


def test_refit_with_the_builds_own_vertices_is_the_identity(mods, forest):
    abi, gb, gi = mods
    objects = gi.pack_objects(forest["pairs"])
    words = gi.refit_objects(objects, (3, 1, 2, 0), forest["vertices"], forest["indices"], forest["rows"][[3, 1, 2, 0]])
    assert words.tolist() == [objects.num_nodes, objects.num_tris, 0, 0]
    assert all(same(a, b) for a, b in zip(download(objects), forest["pairs"]))


def test_guards(mods, forest):
    import torch
    abi, gb, gi = mods
    pairs, rows, moved, indices, alone = (forest[k] for k in ("pairs", "rows", "moved", "indices", "alone"))
    count = lambda ks, j: sum(len(pairs[k][j]) for k in ks)
    # a listed id outside the table (behind it, and negative): flagged, the other listed objects complete and correct
    for bad in (4, -1):
        objects = gi.pack_objects(pairs)
        listed = (SOUP67, bad, SINGLE)
        words = gi.refit_objects(objects, listed, moved, indices, rows[[SOUP67, SOUP1000, SINGLE]], check=False)
        assert words.tolist() == [count((SOUP67, SINGLE), 0), count((SOUP67, SINGLE), 1), gi.BAD_OBJECT, 0]
        got = download(objects)
        assert same(got[SOUP67], alone[SOUP67]) and same(got[SINGLE], alone[SINGLE])
        assert same(got[FLAT], pairs[FLAT]) and same(got[SOUP1000], pairs[SOUP1000])
        with pytest.raises(gb.BuildError, match="object index"):
            gi.refit_objects(objects, listed, moved, indices, rows[[SOUP67, SOUP1000, SINGLE]])
    # one corrupted child id in the 66-node object: flagged, that object incomplete as the model leaves it, the others complete
    broken = pairs[SOUP67][0].copy()
    inner = np.nonzero((broken["child"] > 0).all(1))[0][-1]
    broken["child"][inner, 1] = len(broken) + 5
    model = R.refit(broken, pairs[SOUP67][1], moved, indices[rows[SOUP67][0]:][: rows[SOUP67][1]])
    assert model[2][2] == R.BAD_TOPOLOGY and model[2][0] < len(broken)
    objects = gi.pack_objects([pairs[SINGLE], pairs[FLAT], (broken, pairs[SOUP67][1]), pairs[SOUP1000]])
    listed = LISTS[0]
    words = gi.refit_objects(objects, listed, moved, indices, rows[list(listed)], check=False)
    expect = model[2] + alone[SOUP1000][2] + alone[SINGLE][2]
    assert words.tolist() == [expect[0], expect[1], R.BAD_TOPOLOGY, 0] and words[0] < count(listed, 0)
    got = download(objects)
    assert same(got[SOUP67], model[:2]) and same(got[SOUP1000], alone[SOUP1000]) and same(got[SINGLE], alone[SINGLE])
    assert same(got[FLAT], pairs[FLAT])
    with pytest.raises(gb.BuildError, match="malformed"):
        gi.refit_objects(gi.pack_objects([pairs[SINGLE], pairs[FLAT], (broken, pairs[SOUP67][1]), pairs[SOUP1000]]), listed, moved,
                         indices, rows[list(listed)])
    # a range table whose second stretch leaves the totals, and one whose rows leave the index table: those ranges are flagged and
    # untouched, the others complete
    for field, value in (("node_start", count(listed, 0) - 1), ("first_tri", len(indices) - 1)):
        objects = gi.pack_objects(pairs)
        plan = gi.plan_refit(objects, listed, rows[list(listed)])
        plan.table[field][1] = value
        plan.table_dev = abi.to_device(plan.table, 0)
        words = gi.refit_objects(objects, None, moved, indices, plan, check=False)
        got = download(objects)
        assert words[2] == R.BAD_TOPOLOGY and words[0] == count((SOUP67, SINGLE), 0)
        assert same(got[SOUP1000], pairs[SOUP1000]) and same(got[FLAT], pairs[FLAT])
        assert same(got[SOUP67], alone[SOUP67]) and same(got[SINGLE], alone[SINGLE])
    # host-side refusals enqueue nothing: the objects and the info words stay as they are
    l = abi.lib()
    objects = gi.pack_objects(pairs)
    plan = gi.plan_refit(objects, listed, rows[list(listed)])
    vd, ixd = torch.from_numpy(moved).cuda(), torch.from_numpy(indices).cuda()
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device="cuda")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda dev=0, nv=len(moved), n=len(indices), no=4, nl=3, tn=plan.num_nodes, tr=plan.num_recs, vp=vd.data_ptr(): \
        l.rodent_hip_refit_objects(dev, vp, nv, ixd.data_ptr(), n, objects.nodes.data_ptr(), objects.tris.data_ptr(),
                                   objects.table_dev.data_ptr(), no, plan.table_dev.data_ptr(), nl, tn, tr, scratch.data_ptr(),
                                   info.data_ptr(), stream)
    assert call(n=0) == -1 and call(n=(1 << 25) + 1) == -1 and call(nv=0) == -3 and call(no=0) == gi.ERR_NUM_OBJECTS
    assert call(nl=0) == -11 and call(tn=-1) == -11 and call(tr=-1) == -11 and call(vp=None) == -4 and call(dev=99) == -5
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [77] * 4 and all(same(a, b) for a, b in zip(download(objects), pairs))
    assert l.rodent_hip_refit_objects_plan(None, 4, None, None, None, 3, None, None) == -1
    with pytest.raises(ValueError):
        gi.plan_refit(objects, (), np.zeros((0, 2), np.int32))
    # a clean call afterwards: the flags are per call
    assert call() == 0
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [plan.num_nodes, plan.num_recs, 0, 0]
    assert all(same(a, b) for a, b in zip(download(objects), [alone[k] if k in listed else pairs[k] for k in range(4)]))
