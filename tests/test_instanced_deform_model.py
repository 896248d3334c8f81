"""The CPU model of deforming objects in an instanced scene (tests/instanced_deform_model.py): its restriction to a set D against the
unrestricted rules of scene_update_model, against a corner-by-corner restatement where D shares vertices with static triangles, and its
frame of the deformed test scene beside oracle.render of the same scene baked flat."""
import types

import numpy as np
import pytest

import instanced_deform_model as DM
import instanced_scene_model as IM
import scene_update_model as SU
from conftest import GOLDEN
from rodent_amd import instances as I, scene as S

BOX, CUBE, LAMP = range(3)


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("deform"))
    scene = I.concat_scenes(objects)
    transforms, ids = IM.placements()
    return scene, scene.ranges, transforms, ids, IM.object_bvhs(scene, scene.ranges)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_every_object_deforming_is_the_unrestricted_update(parts):
    scene, ranges, _, _, packed = parts
    ix, nv = scene.indices, len(scene.vertices)
    # the scene has the loader's own tables: the rules reproduce them from the vertices as they are
    fn0 = SU.face_normals(scene.vertices, ix)
    assert same(fn0, scene.face_normals) and same(SU.smooth_normals(fn0, ix, nv), scene.normals)
    assert same(SU.light_records(scene.lights, scene.vertices, ix, scene.materials, scene.light_ids), scene.lights)
    moved = DM.shear_objects(scene, ranges, (BOX, CUBE, LAMP))
    assert not np.array_equal(moved[:, 1], scene.vertices[:, 1]) and np.array_equal(moved[:, 3], scene.vertices[:, 3])
    got = DM.tables(scene, ranges, (LAMP, BOX, CUBE), moved)
    fn = SU.face_normals(moved, ix)
    normals = SU.smooth_normals(fn, ix, nv)
    assert same(got.vertices, moved) and same(got.face_normals, fn) and same(got.normals, normals)
    assert same(got.lights, SU.light_records(scene.lights, moved, ix, scene.materials, scene.light_ids))
    assert same(got.tri_shade, SU.tri_shade(fn, normals, ix))
    assert not same(got.lights, scene.lights) and not same(got.normals, scene.normals)
    given = np.roll(normals, 1, axis=0)
    assert same(DM.tables(scene, ranges, (BOX, CUBE, LAMP), moved, given).normals, given)
    # the hierarchy: every object refitted; with the vertices it was built from it keeps its bytes
    nodes, tris, table, info = DM.hierarchy(packed, ranges, (CUBE, LAMP, BOX), moved, ix)
    assert info.tolist() == [len(packed[0]), len(packed[1]), 0, 0]
    assert same(nodes["child"], packed[0]["child"]) and not same(nodes, packed[0]) and not same(tris, packed[1])
    nodes, tris, table, info = DM.hierarchy(packed, ranges, (CUBE, LAMP, BOX), scene.vertices, ix)
    assert same(nodes, packed[0]) and same(tris, packed[1])


def test_a_static_objects_rows_are_untouched(parts):
    scene, ranges, _, _, packed = parts
    ix = scene.indices
    D = (LAMP, CUBE)
    moved = DM.shear_objects(scene, ranges, D)
    got = DM.tables(scene, ranges, D, moved)
    static = ~DM.in_set(ranges, D, len(ix))
    static_verts = np.unique(ix[static, :3])
    assert static.sum() == ranges[BOX, 1] and same(moved[static_verts], scene.vertices[static_verts])
    assert same(got.face_normals[static], scene.face_normals[static]) and same(got.tri_shade[static], SU.tri_shade(scene.face_normals, scene.normals, ix)[static])
    assert same(got.normals[static_verts], scene.normals[static_verts])
    nl = ranges[BOX, 3]
    assert nl > 0 and same(got.lights[:nl], scene.lights[:nl]) and not same(got.lights[nl:], scene.lights[nl:])
    assert not same(got.face_normals[~static], scene.face_normals[~static])
    nodes, tris, table, info = DM.hierarchy(packed, ranges, D, moved, ix)
    box = table[BOX]
    ns, ts = slice(box["node_offset"], box["node_offset"] + box["num_nodes"]), slice(box["tri_offset"], box["tri_offset"] + box["num_tris"])
    assert same(nodes[ns], packed[0][ns]) and same(tris[ts], packed[1][ts])
    assert info.tolist() == [table["num_nodes"][list(D)].sum(), table["num_tris"][list(D)].sum(), 0, 0]
    for o in D:
        row = table[o]
        ns = slice(row["node_offset"], row["node_offset"] + row["num_nodes"])
        assert not same(nodes[ns], packed[0][ns]), o


def test_a_vertex_shared_with_a_static_triangle_sums_its_stored_face_normal():
    """Two `objects` over ONE vertex pool (scene_update_model.indexed_soup: from 140 triangles on, a fan of 70 around vertex 0), the
    second one deforming: every vertex it names, restated corner by corner in ascending (triangle, corner) order."""
    v, ix, light_ids, lights = SU.indexed_soup(200, 7)
    n, nv = len(ix), len(v)
    scene = types.SimpleNamespace(vertices=v, indices=ix, light_ids=light_ids, lights=lights,
                                  materials=np.zeros(2, S.MATERIAL), face_normals=SU.face_normals(v, ix))
    scene.materials["emissive"][1] = 1
    scene.normals = SU.smooth_normals(scene.face_normals, ix, nv)
    # stored face normals that the rules would NOT reproduce mark what is read and what is recomputed
    scene.face_normals[:, :3] = scene.face_normals[:, [1, 2, 0]]
    ranges = np.int32([[0, 50, 0, len(lights)], [50, n - 50, len(lights), 0]])
    moved = SU.shear(v)
    got = DM.tables(scene, ranges, (1,), moved)
    fresh = SU.face_normals(moved, ix)
    assert same(got.face_normals[:50], scene.face_normals[:50]) and same(got.face_normals[50:], fresh[50:])
    named = np.unique(ix[50:, :3])
    shared = np.intersect1d(named, np.unique(ix[:50, :3]))
    assert len(shared) > 10 and 0 in shared and len(named) < nv
    for vert in named:
        s = np.zeros(3, np.float32)
        with np.errstate(all="ignore"):
            for t in range(n):
                for k in range(3):
                    if ix[t, k] == vert:
                        s = s + (scene.face_normals[t, :3] if t < 50 else fresh[t, :3])
            l2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
            want = np.float32([0, 1, 0, 0])
            if l2 > np.finfo(np.float32).eps:
                want[:3] = s * (np.float32(1) / np.sqrt(l2))
        assert got.normals[vert].tobytes() == want.tobytes(), vert
    others = np.setdiff1d(np.arange(nv), named)
    assert same(got.normals[others], scene.normals[others])
    # the lights all belong to the static object: none moves
    assert same(got.lights, lights)


def test_model_frame_of_the_deformed_scene_matches_the_flat_oracle(parts, oracle):
    """As test_instanced_scene_model.test_model_frame_matches_the_flat_oracle, for the scene with the cube and the lamp sheared: the
    model's frame beside oracle.render of the deformed scene baked flat, held to that test's bound."""
    scene, ranges, t, ids, packed = parts
    D = (CUBE, LAMP)
    moved = DM.shear_objects(scene, ranges, D)
    deformed = DM.tables(scene, ranges, D, moved)
    refitted = DM.hierarchy(packed, ranges, D, moved, scene.indices)
    cam = S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, IM.W, IM.H)
    f = DM.frame(deformed, ranges, t, ids, refitted, cam, 0, IM.SPP, IM.MAXLEN, IM.W, IM.H)
    flat = IM.with_flat_bvh(IM.baked(deformed, ranges, t, ids))
    film, counts = oracle.render(flat, cam, 0, IM.SPP, IM.MAXLEN, IM.W, IM.H)
    a, b = oracle.tonemap(f.film, 1).astype(np.float32), oracle.tonemap(film, 1).astype(np.float32)
    mse = ((a - b) ** 2).mean() / 255.0 ** 2
    print("tone-mapped MSE", mse, "counts", f.counts, counts)
    assert mse < 3e-4, mse
    assert f.film.mean() > 0.02
    # the deformed objects are seen: camera rays hit triangles of every instance of D
    rays, pixels, hits, inst_ids = f.primary[0]
    assert set(np.unique(inst_ids[hits["tri_id"] >= 0])) >= {0, 1, 2, 5, 6}
