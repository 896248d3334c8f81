"""Geometry that deforms inside the objects of an instanced scene (rodent_hip_scene_deform_prepare / _device / _status;
Renderer.prepare_deform / deform_objects / deform_status) against tests/instanced_deform_model.py, on the test scene of
tests/instanced_scene_model.py: the Cornell box once (static), the cube four times and the emissive quad twice (D = {cube, lamp}).

Every table instance_tables(), scene_tables() and scene_bvh() expose is compared byte for byte with the model after a shear of D's
vertices, after a second deform that also moves the instances, and after two deforms on two streams; with smooth and with given
normals; a deform with unmoved vertices keeps every byte; a frame equals the model's frame; every refusal of the prepare call leaves
the loaded scene rendering the same frame; a non-finite vertex comes back as a status and the next sound call is clean.  What a deform
writes for D is a function of the new vertices and of the static objects' stored rows alone, so the model always starts from the scene
as it was created."""
import contextlib

import numpy as np
import pytest

import instanced_deform_model as DM
import instanced_scene_model as IM
from conftest import GOLDEN
from rodent_amd import instances as I, scene as S

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = IM.W, IM.H, IM.SPP, IM.MAXLEN
BOX, CUBE, LAMP = range(3)
D = (LAMP, CUBE)


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


class Parts:
    pass


@pytest.fixture(scope="module")
def parts(native_build, tmp_path_factory):
    p = Parts()
    objects = IM.scene_objects(GOLDEN, tmp_path_factory.mktemp("deform"))
    p.scene, p.cornell = I.concat_scenes(objects), objects[0]
    p.ranges = p.scene.ranges
    p.transforms, p.ids = IM.placements()
    p.moved_transforms = IM.placements(moved=True)[0]
    p.hierarchy = IM.object_bvhs(p.scene, p.ranges)
    p.sheared = DM.shear_objects(p.scene, p.ranges, D)
    p.sheared_more = DM.shear_objects(p.scene, p.ranges, D, kx=-0.15, kz=0.3, ky=-0.1)
    return p


@pytest.fixture(scope="module")
def cam():
    return S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)


@contextlib.contextmanager
def rendering(R, parts, **kw):
    r = R.Renderer(parts.scene, W, H, SPP, MAXLEN, instances=(parts.ranges, parts.transforms, parts.ids), **kw)
    try:
        yield r
    finally:
        r.close()


def expected(parts, vertices, transforms, normals=None):
    """What the three table getters must show after D took `vertices` under `transforms`: (instance tables, scene tables, (nodes,
    tris), the refit's info words), and the deformed scene with its hierarchy for a frame."""
    deformed = DM.tables(parts.scene, parts.ranges, D, vertices, normals)
    nodes, tris, table, refit_info = DM.hierarchy(parts.hierarchy, parts.ranges, D, vertices, parts.scene.indices)
    tlas, inst, info = IM.tlas_of(nodes, table, transforms, parts.ids)
    world = IM.world_lights(deformed.lights, parts.ranges, transforms, parts.ids)
    instance_tables = {"tlas_nodes": tlas, "instances": inst, "slot_of": IM.slot_of(inst), "bases": IM.bases(parts.ranges, parts.ids),
                       "lights": world, "object_lights": deformed.lights, "light_owner": IM.light_owner(parts.ranges, parts.ids),
                       "objects": table, "tlas_info": info}
    scene_tables = {"vertices": deformed.vertices, "normals": deformed.normals, "face_normals": deformed.face_normals, "lights": world,
                    "tri_shade": deformed.tri_shade}
    return instance_tables, scene_tables, (nodes, tris), refit_info, deformed


def assert_state(r, parts, want, what, transforms):
    instance_tables, scene_tables, bvh, refit_info, _ = want
    flags, refit_words, tlas_words = r.deform_status()
    assert (flags, refit_words, tlas_words) == (0, refit_info.tolist(), instance_tables["tlas_info"].tolist()), what
    got = r.instance_tables()
    for name, w in instance_tables.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: instance table `{name}`"
    assert np.array_equal(got["descs"]["object_to_world"], transforms) and np.array_equal(got["descs"]["object"], parts.ids), what
    got = r.scene_tables()
    assert got["top_image"] is None and got["top_image_large"] is None
    for name, w in scene_tables.items():
        g = got[name]
        if name == "tri_shade" and g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: scene table `{name}`"
    nodes, tris = r.scene_bvh()
    assert nodes.tobytes() == bvh[0].tobytes() and tris.tobytes() == bvh[1].tobytes(), f"{what}: the packed hierarchy"


def test_tables_equal_the_model_after_deforms_with_smooth_normals(R, parts, cam):
    import torch
    first = expected(parts, parts.sheared, parts.transforms)
    second = expected(parts, parts.sheared_more, parts.moved_transforms)
    assert first[3].tolist()[2:] == [0, 0] and first[1]["tri_shade"].tobytes() != second[1]["tri_shade"].tobytes()
    with rendering(R, parts) as r:
        created = (r.instance_tables(), r.scene_tables(), r.scene_bvh())
        r.prepare_deform(D)
        assert r.deform_status()[0] == 0
        v1, v2 = torch.from_numpy(parts.sheared).cuda(), torch.from_numpy(parts.sheared_more).cuda()
        m = torch.from_numpy(parts.moved_transforms).cuda()
        r.deform_objects(v1)
        assert_state(r, parts, first, "after a shear of D", parts.transforms)
        # the static object's rows, as they were created
        static = ~DM.in_set(parts.ranges, D, parts.scene.num_tris)
        assert r.scene_tables()["face_normals"][static].tobytes() == created[1]["face_normals"][static].tobytes()
        nb = int(created[0]["objects"][BOX]["num_nodes"])
        assert r.scene_bvh()[0][:nb].tobytes() == created[2][0][:nb].tobytes()
        assert r.scene_bvh()[0][nb:].tobytes() != created[2][0][nb:].tobytes()
        r.deform_objects(v2, transforms=m)
        assert_state(r, parts, second, "after a second deform with new matrices", parts.moved_transforms)
        # two deforms on two streams, no check in between (nothing waits): the frame behind them sees the second one
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r.deform_objects(v1, transforms=torch.from_numpy(parts.transforms).cuda(), stream=s1, check=False)
        r.deform_objects(v2, transforms=m, stream=s2, check=False)
        r.render(cam, 0)
        assert r.film().mean() > 0.02
        assert_state(r, parts, second, "after two deforms on two streams", parts.moved_transforms)
        # identity: the scene's own table, unmoved (nothing is copied), keeps every byte, the top-level hierarchy included
        own = r.scene_vertices_tensor()
        assert own.data_ptr() == r.scene_table_pointers()["vertices"]
        r.deform_objects(own)
        assert_state(r, parts, second, "after a deform with unmoved vertices", parts.moved_transforms)
        # written in place with torch ops: back to the first shear under the matrices as they are
        own.copy_(v1)
        r.deform_objects(own)
        assert_state(r, parts, expected(parts, parts.sheared, parts.moved_transforms), "after an in-place write", parts.moved_transforms)


def test_tables_equal_the_model_with_given_normals(R, parts):
    import torch
    # D's rows from somewhere else (the smooth normals of the other shear); every other row the scene's
    named = np.unique(parts.scene.indices[DM.in_set(parts.ranges, D, parts.scene.num_tris), :3])
    normals = np.array(parts.scene.normals, np.float32)
    normals[named] = DM.tables(parts.scene, parts.ranges, D, parts.sheared_more).normals[named]
    want = expected(parts, parts.sheared, parts.transforms, normals)
    assert want[1]["normals"].tobytes() != expected(parts, parts.sheared, parts.transforms)[1]["normals"].tobytes()
    with rendering(R, parts) as r:
        r.prepare_deform(D, smooth_normals=False)
        r.deform_objects(torch.from_numpy(parts.sheared).cuda(), torch.from_numpy(normals).cuda())
        assert_state(r, parts, want, "with given normals", parts.transforms)
        r.prepare_deform(D[::-1])                                            # the set replaced by itself in another order, now smooth
        r.deform_objects(torch.from_numpy(parts.sheared).cuda())
        assert_state(r, parts, expected(parts, parts.sheared, parts.transforms), "after the set was replaced", parts.transforms)


@pytest.fixture(scope="module")
def model_frame(parts, oracle, cam):
    *_, deformed = want = expected(parts, parts.sheared, parts.transforms)
    nodes, tris = want[2]
    return DM.frame(deformed, parts.ranges, parts.transforms, parts.ids, (nodes, tris, parts.hierarchy[2]), cam, 0, SPP, MAXLEN, W, H)


def test_frame_equals_the_model(R, parts, model_frame, cam):
    import torch
    with rendering(R, parts, capacity=4096) as r:
        r.render(cam, 0)
        before = r.film()
        r.prepare_deform(D)
        r.deform_objects(torch.from_numpy(parts.sheared).cuda(), check=False)      # the frame is ordered behind it by the event
        r.clear()
        r.render(cam, 0)
        c = r.counters()
        film = r.film()
        assert r.deform_status()[0] == 0 and c["iterations"] > 3
    assert (c["primary_rays"], c["shadow_rays"], c["generated"]) == (model_frame.counts[0], model_frame.counts[1], W * H * SPP)
    assert np.allclose(film, model_frame.film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02
    assert not np.allclose(film, before, rtol=FILM_RTOL, atol=FILM_ATOL)


def test_refusals_of_prepare_leave_the_scene_as_it_is(R, parts, cam):
    import torch
    from rodent_amd import gpubuild
    refused = (((), "no objects"), ((3,), "outside the table"), ((CUBE, -1), "outside the table"), ((CUBE, LAMP, CUBE), "twice"))
    flat = R.Renderer(parts.cornell, W, H, SPP, MAXLEN)
    try:
        flat.render(cam, 0)
        film = flat.film()
        with pytest.raises(gpubuild.BuildError, match="no instanced scene"):
            flat.prepare_deform(D)
        flat.clear(); flat.render(cam, 0)
        assert np.allclose(flat.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.01
    finally:
        flat.close()
    with rendering(R, parts) as r:
        r.render(cam, 0)
        film = r.film()
        for ids, why in refused:
            with pytest.raises(gpubuild.BuildError, match=why):
                r.prepare_deform(ids)
        r.clear(); r.render(cam, 0)
        assert np.allclose(r.film(), film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02
        # an earlier set stays too
        r.prepare_deform(D)
        for ids, why in refused:
            with pytest.raises(gpubuild.BuildError, match=why):
                r.prepare_deform(ids)
        r.deform_objects(torch.from_numpy(parts.sheared).cuda())
        assert_state(r, parts, expected(parts, parts.sheared, parts.transforms), "after refused prepare calls", parts.transforms)


def test_a_non_finite_vertex_is_a_status_and_the_next_sound_call_is_clean(R, parts):
    import torch
    from rodent_amd import gpubuild
    bad = parts.sheared.copy()
    cube_vertex = parts.scene.indices[parts.ranges[CUBE, 0], 0]
    bad[cube_vertex, 1] = np.nan
    with rendering(R, parts) as r:
        r.prepare_deform(D)
        r.deform_objects(torch.from_numpy(bad).cuda(), check=False)
        flags, refit_words, _ = r.deform_status()
        assert flags & gpubuild.NON_FINITE and refit_words[2] & gpubuild.NON_FINITE
        with pytest.raises(gpubuild.BuildError, match="non-finite"):
            r.deform_objects(torch.from_numpy(bad).cuda())
        r.deform_objects(torch.from_numpy(parts.sheared).cuda())
        assert_state(r, parts, expected(parts, parts.sheared, parts.transforms), "after a sound call", parts.transforms)
