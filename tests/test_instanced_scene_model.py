"""The CPU model of instanced scenes in the renderer (tests/instanced_scene_model.py) against fp64 and against the flat oracle: the
world light table, the normal map N, and the model's frame of the test scene beside oracle.render of the same scene baked flat."""
import numpy as np
import pytest

import instanced_scene_model as IM
import instance_model as M
from conftest import GOLDEN
from rodent_amd import instances as I, scene as S

EPS = 2.0 ** -24                                   # unit roundoff of float32


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("instanced"))
    scene = I.concat_scenes(objects)
    transforms, ids = IM.placements()
    return scene, scene.ranges, transforms, ids


def test_concatenation_keeps_every_object_its_tables(parts):
    scene, ranges, _, _ = parts
    assert ranges[:, 0].tolist() == [0, ranges[0, 1], ranges[0, 1] + 12] and ranges[1:, 1].tolist() == [12, 2]
    assert ranges[:, 2].tolist() == [0, ranges[0, 3], ranges[0, 3]] and ranges[2, 3] == 2 and ranges[1, 3] == 0
    for first, n, first_light, num_lights in ranges:
        ind = scene.indices[first:first + n]
        emissive = scene.materials["emissive"][ind[:, 3]] != 0
        ids = scene.light_ids[first:first + n]
        assert ((ids[emissive] >= first_light) & (ids[emissive] < first_light + num_lights)).all() and (ids[~emissive] == 0).all()
    assert scene.indices[:, :3].max() == len(scene.vertices) - 1 and scene.indices[:, 3].max() == len(scene.materials) - 1


def test_world_lights_against_fp64(parts):
    """Areas and normals of the world lights beside an fp64 evaluation of the same geometry.  Bounds, per light: a mapped corner is a
    four-term sum, off by at most 4 EPS times its terms' magnitudes (<= 4 EPS P, P the largest |term| sum over the corners); an edge
    inherits twice that plus its own rounding, so its relative error is (8 P / |e| + 1) EPS and the area's (two edges, the cross
    product's and the square root's own roundings, the two divisions) stays below (16 P / e_min + 12) EPS.  A normal component is a
    three-term sum of products with the rounded inverse: (3 + 1) EPS times the sum of its terms' magnitudes S, then the normalisation's
    4 EPS: |n - n64| <= (4 S / |n'| + 4) EPS per component."""
    scene, ranges, t, ids = parts
    got = IM.world_lights(scene.lights, ranges, t, ids)
    owner = IM.light_owner(ranges, ids)
    assert len(got) == ranges[ids, 3].sum() == ranges[0, 3] + 4
    src = np.arange(len(owner)) - IM.bases(ranges, ids)[owner, 1]
    m = t.astype(np.float64).reshape(-1, 3, 4)[owner]
    lin, tr = m[:, :, :3], m[:, :, 3]
    obj = scene.lights[src]
    p = [np.einsum("nab,nb->na", lin, obj[k][:, :3].astype(np.float64)) + tr for k in ("v0", "v1", "v2")]
    mag = np.max([np.einsum("nab,nb->na", np.abs(lin), np.abs(obj[k][:, :3].astype(np.float64))) + np.abs(tr)
                  for k in ("v0", "v1", "v2")], axis=(0, 2))
    e1, e2 = p[1] - p[0], p[2] - p[0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    e_min = np.minimum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))
    rel = np.abs(got["inv_area"].astype(np.float64) * area - 1.0)
    assert (rel <= (16 * mag / e_min + 12) * EPS).all(), (rel / EPS, mag / e_min)
    inv_t = np.linalg.inv(lin).transpose(0, 2, 1)
    n_obj = obj["n"].astype(np.float64)
    n64 = np.einsum("nab,nb->na", inv_t, n_obj)
    terms = np.einsum("nab,nb->na", np.abs(inv_t), np.abs(n_obj)).max(axis=1)
    length = np.linalg.norm(n64, axis=1)
    n64 /= length[:, None]
    assert (np.abs(got["n"] - n64).max(axis=1) <= (4 * terms / length + 4) * EPS).all()
    # the emitting side: N(n) keeps the side the object's own normal had relative to its corners, the cross product of the mapped
    # corners changes sides under a mirroring matrix
    side_obj = np.einsum("na,na->n", np.cross(obj["v1"][:, :3] - obj["v0"][:, :3], obj["v2"][:, :3] - obj["v0"][:, :3]), obj["n"])
    side_world = np.einsum("na,na->n", np.cross(e1, e2), got["n"].astype(np.float64))
    mirrored = np.linalg.det(lin) < 0
    assert mirrored.any() and (~mirrored).any()
    assert (np.sign(side_world) == np.where(mirrored, -1, 1) * np.sign(side_obj)).all()
    assert (got["n"][owner >= 5][:, 1] < -0.9).all()                     # both quads still shine down into the room
    # colours and the corners' fourth words are copies
    assert np.array_equal(got["color"], obj["color"]) and all(np.array_equal(got[k][:, 3], obj[k][:, 3]) for k in ("v0", "v1", "v2"))


def test_mapped_face_normals_stay_orthogonal_to_the_mapped_edges(parts):
    """N(fn) . (mapped edge) is zero in exact arithmetic (fn . e = 0 and N is the inverse transpose).  In float32: the stored fn is
    off the true normal by ~2 EPS, N(fn) by 4 EPS of its terms and its normalisation by 4 more, a mapped edge by 8 EPS P (above):
    |dot| <= (16 |e| + 16 P) EPS suffices for unit normals, with P the largest corner magnitude sum of the triangle."""
    scene, ranges, t, ids = parts
    b = IM.baked(scene, ranges, t, ids)
    v = b.vertices[:, :3].astype(np.float64).reshape(-1, 3, 3)
    fn = b.face_normals[:, :3].astype(np.float64)
    assert np.allclose(np.linalg.norm(fn, axis=1), 1.0, atol=4 * EPS)
    P = np.abs(v).sum(axis=2).max(axis=1)
    for a, c in ((0, 1), (0, 2), (1, 2)):
        e = v[:, c] - v[:, a]
        dot = np.abs(np.einsum("na,na->n", fn, e))
        assert (dot <= (16 * np.linalg.norm(e, axis=1) + 16 * P) * EPS).all()


def test_tables_follow_the_rules(parts):
    scene, ranges, t, ids = parts
    b = IM.bases(ranges, ids)
    assert b[:, 0].tolist() == ranges[ids, 0].tolist()
    nl = ranges[0, 3]
    assert b[:, 1].tolist() == [0, nl - nl, nl - nl, nl - nl, nl - nl, nl - ranges[2, 2], nl + 2 - ranges[2, 2]]
    nodes, tris, table = IM.object_bvhs(scene, ranges)
    tlas, inst, info = IM.tlas_of(nodes, table, t, ids)
    so = IM.slot_of(inst)
    assert sorted(so.tolist()) == list(range(7)) and ((inst["instance_id"][so] & 0x7FFFFFFF) == np.arange(7)).all()


@pytest.fixture(scope="module")
def model_frame(parts, oracle):
    scene, ranges, t, ids = parts
    cam = S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, IM.W, IM.H)
    return cam, IM.frame(scene, ranges, t, ids, IM.object_bvhs(scene, ranges), cam, 0, IM.SPP, IM.MAXLEN, IM.W, IM.H)


def test_model_frame_matches_the_flat_oracle(parts, oracle, model_frame):
    """The model's frame beside oracle.render of the scene baked flat under a flat BVH2: two renderers that agree statistically, not
    bitwise (a hit's t, u, v come from the object-space intersection in one and the world-space one in the other), held to the bound
    test_cornell_matches_reference_image_full_size uses for such a pair."""
    scene, ranges, t, ids = parts
    cam, f = model_frame
    flat = IM.with_flat_bvh(IM.baked(scene, ranges, t, ids))
    film, counts = oracle.render(flat, cam, 0, IM.SPP, IM.MAXLEN, IM.W, IM.H)
    a, b = oracle.tonemap(f.film, 1).astype(np.float32), oracle.tonemap(film, 1).astype(np.float32)
    mse = ((a - b) ** 2).mean() / 255.0 ** 2
    print("tone-mapped MSE", mse, "counts", f.counts, counts)
    assert mse < 3e-4, mse
    assert f.film.mean() > 0.02
    # every class of instance is seen by camera rays, and the coincident pair answers with the later instance of its leaf order
    rays, pixels, hits, inst_ids = f.primary[0]
    assert set(np.unique(inst_ids[hits["tri_id"] >= 0])) >= {0, 1, 2, 5, 6} and ({3, 4} & set(inst_ids.tolist()))
