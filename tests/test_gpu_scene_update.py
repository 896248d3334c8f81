"""The device scene update (rodent_hip_scene_refit_device, csrc/render_update.h; Renderer.update_geometry_device) on the GPU.

The host entry (rodent_hip_scene_refit / Renderer.update_geometry), fed tests/scene_update_model.py's tables, is what it is checked
against: after either path every table the scene owns (scene_tables(), scene_bvh()) holds the same bytes.

* the Cornell box under device hierarchies of max_leaf 1, 2 and 8, after a shear;
* indexed soups of 1 ... 1000 triangles with shared vertices, a 70-triangle fan, an unused vertex, several emitters (two naming one
  light, one light named by nobody) and trees past 31 and past 255 nodes; the 65-triangle soup has a triangle that names a vertex
  twice: NaN equals NaN there, bits otherwise;
* the caller's normals are kept bit for bit; the scene's own vertex table written in place gives the same tables as a separate buffer;
* render, refit, render without a synchronisation in between: the second film is the oracle's film of the moved scene (both mappings);
* two refits on two streams end in the state of the second; repeated calls and other streams give identical bytes;
* the status entry reports a non-finite coordinate without aborting; the identity on the atrium.
"""
import copy
import types

import numpy as np
import pytest

import scene_update_model as M
from conftest import GOLDEN
from rodent_amd import formats as F
from rodent_amd import scene as S

pytestmark = pytest.mark.gpu
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                  # test_gpu_refit.py's
SOUPS = (1, 2, 3, 63, 64, 65, 257, 1000)
TWICE = 65                                         # the soup with a triangle naming one vertex twice
W = H = 32
# table -> the words of a record that are floats (NaN may meet NaN there); every other word is compared as bits
FLOAT_WORDS = {"vertices": 4, "normals": 4, "face_normals": 4, "tri_shade": 12, "lights": 20, "top_image": 12, "top_image_large": 12,
               "nodes": 12, "tris": None}


@pytest.fixture(scope="module")
def Rn(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available(), "these tests need a GPU"
    return render


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


def soup_scene(n, seed=None, twice=False):
    v, ix, light_ids, lights = M.indexed_soup(n, n + 1 if seed is None else seed, twice)
    sc = types.SimpleNamespace(vertices=v, indices=ix, light_ids=light_ids, num_tris=n)
    sc.materials = np.zeros(2, S.MATERIAL)
    sc.materials["kd"][0] = 0.6; sc.materials["type"][0] = 1
    sc.materials["emissive"][1] = 1
    sc.nodes, sc.tris = np.zeros(0, F.NODE2), np.zeros(0, F.TRI1)
    sc.texcoords = np.zeros((len(v), 4), np.float32)
    sc.textures, sc.texels = np.zeros(0, S.TEXTURE), np.zeros(0, np.uint32)
    sc.lights = lights
    return with_model_tables(sc, v)


def with_model_tables(scene, vertices, normals=None):
    """`scene` with `vertices` and the model's face normals, vertex normals (or `normals`) and light records."""
    out = copy.copy(scene)
    out.vertices = np.ascontiguousarray(vertices, np.float32)
    out.face_normals = M.face_normals(out.vertices, scene.indices)
    out.normals = M.smooth_normals(out.face_normals, scene.indices, len(out.vertices)) if normals is None else normals
    out.lights = M.light_records(scene.lights, out.vertices, scene.indices, scene.materials, scene.light_ids)
    return out


def collect(r):
    tables = r.scene_tables()
    tables["nodes"], tables["tris"] = r.scene_bvh()
    return tables


def assert_same_tables(got, want, nan_ok=False, what=""):
    assert set(got) == set(want) == set(FLOAT_WORDS)
    for name, a in got.items():
        b = want[name]
        assert a is not None and b is not None and a.shape == b.shape, (what, name)
        if nan_ok:
            record = a.dtype.itemsize // 4 if a.dtype.names else a.shape[-1]
            ua, ub = (x.reshape(-1).view(np.uint32).reshape(-1, record) for x in (a, b))
            floats = np.zeros(record, bool)
            if name == "tris":
                floats[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = True
            else:
                floats[:FLOAT_WORDS[name]] = True
            both_nan = np.isnan(ua.view(np.float32)) & np.isnan(ub.view(np.float32)) & floats
            assert ((ua == ub) | both_nan).all(), (what, name)
        else:
            assert a.tobytes() == b.tobytes(), (what, name)


def device_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_paths(Rn, scene, moved, normals=None, **renderer):
    """The tables after update_geometry(moved) and after update_geometry_device(moved.vertices[, normals]), each on a fresh renderer."""
    r = Rn.Renderer(scene, W, H, 1, 4, **renderer)
    try:
        r.update_geometry(moved)
        host = collect(r)
    finally:
        r.close()
    r = Rn.Renderer(scene, W, H, 1, 4, **renderer)
    try:
        before = collect(r)
        r.update_geometry_device(device_tensor(moved.vertices), None if normals is None else device_tensor(normals))
        assert r.update_status() == (0, [len(before["nodes"]), len(before["tris"]), 0, 0])
        device = collect(r)
    finally:
        r.close()
    assert device["nodes"]["child"].tobytes() == before["nodes"]["child"].tobytes()
    assert device["vertices"].tobytes() != before["vertices"].tobytes()
    return host, device


@pytest.mark.parametrize("max_leaf", (1, 2, 8))
def test_cornell_tables_equal_the_host_paths(Rn, cornell_scene, max_leaf):
    moved = with_model_tables(cornell_scene, M.shear(cornell_scene.vertices))
    host, device = both_paths(Rn, cornell_scene, moved, gpu_bvh=max_leaf)
    assert all(not np.isnan(device[n]).any() for n in ("normals", "face_normals", "tri_shade"))
    assert_same_tables(device, host, what=f"cornell max_leaf {max_leaf}")
    assert device["vertices"].tobytes() == moved.vertices.tobytes() and device["lights"].tobytes() == moved.lights.tobytes()


@pytest.mark.parametrize("n", SOUPS)
def test_soup_tables_equal_the_host_paths(Rn, n):
    scene = soup_scene(n, twice=n == TWICE)
    moved = with_model_tables(scene, M.shear(scene.vertices))
    host, device = both_paths(Rn, scene, moved, gpu_bvh=1)
    assert len(device["nodes"]) == max(1, n - 1)
    nans = int(np.isnan(device["face_normals"]).sum())
    assert nans == (3 if n == TWICE else 0)
    assert_same_tables(device, host, nan_ok=n == TWICE, what=f"soup {n}")
    # the model itself, where a host path could only agree with the device by accident
    assert device["normals"].tobytes() == moved.normals.tobytes()
    assert device["lights"].tobytes() == moved.lights.tobytes() and device["lights"][-1].tobytes() == scene.lights[-1].tobytes()
    for name, capacity in (("top_image", 31), ("top_image_large", 255)):
        assert device[name].tobytes() == M.top_image(device["nodes"], capacity).tobytes(), name
    if n >= 140:
        first, _ = M.incidence(scene.indices, len(scene.vertices))
        assert first[1] - first[0] >= 70 and first[-1] == first[-2]


def test_the_callers_normals_are_kept(Rn):
    scene = soup_scene(257)
    rng = np.random.default_rng(3)
    normals = np.zeros((len(scene.vertices), 4), np.float32)
    normals[:, :3] = rng.normal(size=(len(normals), 3)).astype(np.float32)
    moved = with_model_tables(scene, M.shear(scene.vertices), normals)
    host, device = both_paths(Rn, scene, moved, normals=normals, gpu_bvh=1)
    assert device["normals"].tobytes() == normals.tobytes()
    assert device["tri_shade"].tobytes() == M.tri_shade(moved.face_normals, normals, scene.indices).tobytes()
    assert_same_tables(device, host, what="caller's normals")


def test_the_scenes_own_vertex_table_written_in_place(Rn):
    import torch
    scene = soup_scene(257)
    results = []
    for in_place in (False, True):
        r = Rn.Renderer(scene, W, H, 1, 4, gpu_bvh=1)
        try:
            if in_place:
                v = r.scene_vertices_tensor()
                assert v.data_ptr() == r.scene_table_pointers()["vertices"]
                x, z = v[:, 0] + 0.25 * v[:, 1], v[:, 2] + float(np.float32(0.1)) * v[:, 1]
                v[:, 0], v[:, 2] = x, z                              # a torch op writes the scene's own table
                r.update_geometry_device(v)
            else:
                r.update_geometry_device(device_tensor(M.shear(scene.vertices)))
            results.append(collect(r))
        finally:
            r.close()
    assert results[1]["vertices"].tobytes() == M.shear(scene.vertices).tobytes()
    assert_same_tables(results[1], results[0], what="in place")


@pytest.mark.parametrize("mapping", ("streaming", "megakernel"))
def test_render_refit_render_without_a_synchronisation(Rn, oracle, cornell_scene, mapping):
    import torch
    W2, H2, spp, depth = 64, 64, 4, 6
    cam = S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W2, H2)
    moved = with_model_tables(cornell_scene, M.shear(cornell_scene.vertices))
    r = Rn.Renderer(cornell_scene, W2, H2, spp, depth, gpu_bvh=2, mapping=mapping)
    try:
        assert r.mapping_name() == mapping
        r.prepare_update()
        side = torch.cuda.Stream()
        v = device_tensor(moved.vertices)
        r.render(cam, 0)                                             # the frame in front of the refit
        film_first = r.film()
        r.clear()
        r.update_geometry_device(v, stream=side, check=False)       # enqueued on another stream; nobody waits for it ...
        r.render(cam, 0)                                             # ... but the frame behind it, on the null stream
        film = r.film()
        nodes, tris = r.scene_bvh()
        assert r.update_status()[0] == 0
    finally:
        r.close()
    refitted = copy.copy(moved)
    refitted.nodes, refitted.tris = nodes, tris                      # the moved scene under the hierarchy the device traces
    film_o, _ = oracle.render(refitted, cam, 0, spp, depth, W2, H2)
    assert np.allclose(film, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.01
    assert not np.allclose(film, film_first, rtol=FILM_RTOL, atol=FILM_ATOL)


def test_two_refits_on_two_streams_end_in_the_second(Rn):
    import torch
    scene = soup_scene(1000)
    first, second = M.shear(scene.vertices), M.shear(scene.vertices, -0.3, 0.45)
    r = Rn.Renderer(scene, W, H, 1, 4, gpu_bvh=1)
    try:
        r.update_geometry_device(device_tensor(second))
        alone = collect(r)
        a, b = device_tensor(first), device_tensor(second)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(3):
            r.update_geometry_device(a, stream=s1, check=False)
            r.update_geometry_device(b, stream=s2, check=False)
        assert r.update_status()[0] == 0
        assert_same_tables(collect(r), alone, what="second of two")
        r.update_geometry_device(a, stream=s2, check=False)
        r.update_geometry_device(b, stream=None, check=False)
        r.update_geometry_device(a, stream=s1, check=False)
        after_first = collect(r)
    finally:
        r.close()
    assert alone["vertices"].tobytes() == second.tobytes() and after_first["vertices"].tobytes() == first.tobytes()
    assert after_first["face_normals"].tobytes() == M.face_normals(first, scene.indices).tobytes()


def test_repeated_calls_and_other_streams_give_identical_bytes(Rn):
    import torch
    scene = soup_scene(257)
    v = M.shear(scene.vertices)
    results = []
    for stream in (None, "new"):
        r = Rn.Renderer(scene, W, H, 1, 4, gpu_bvh=2)
        try:
            t = device_tensor(v)
            for _ in range(2):
                r.update_geometry_device(t, stream=torch.cuda.Stream() if stream else None)
                results.append(collect(r))
        finally:
            r.close()
    for other in results[1:]:
        assert_same_tables(other, results[0], what="determinism")


def test_status_reports_a_non_finite_coordinate_without_aborting(Rn):
    from rodent_amd import gpubuild
    scene = soup_scene(64)
    r = Rn.Renderer(scene, W, H, 1, 4, gpu_bvh=1)
    try:
        nn, nt = (len(x) for x in r.scene_bvh())
        assert r.update_status() == (0, [nn, nt, 0, 0])              # before the first refit
        r.update_geometry_device(device_tensor(M.shear(scene.vertices)))
        assert r.update_status() == (0, [nn, nt, 0, 0])
        topology = r.scene_bvh()[0]["child"].copy()
        bad = M.shear(scene.vertices)
        bad[scene.indices[5, 1], 2] = np.inf
        r.update_geometry_device(device_tensor(bad), check=False)
        flags, words = r.update_status()
        assert flags == gpubuild.NON_FINITE and words == [nn, nt, gpubuild.NON_FINITE, 0]
        assert r.scene_bvh()[0]["child"].tobytes() == topology.tobytes()
        with pytest.raises(gpubuild.BuildError, match="non-finite"):
            r.update_geometry_device(device_tensor(bad))
        r.update_geometry_device(device_tensor(M.shear(scene.vertices)))          # the flags are per call
        assert r.update_status() == (0, [nn, nt, 0, 0])
        with pytest.raises(ValueError):
            r.update_geometry_device(device_tensor(bad[:-1]))
    finally:
        r.close()


def test_identity_on_the_atrium(Rn, tmp_path_factory):
    from rodent_amd import scenes
    atrium = S.convert(scenes.scene_obj("atrium"), tmp_path_factory.mktemp("atrium") / "atrium.rscene")
    r = Rn.Renderer(atrium, W, H, 1, 4, gpu_bvh=2)
    try:
        before = collect(r)
        r.update_geometry_device(r.scene_table_pointers()["vertices"])
        assert r.update_status()[0] == 0
        after = collect(r)
    finally:
        r.close()
    for name in ("vertices", "face_normals", "lights", "nodes", "tris"):
        assert after[name].tobytes() == before[name].tobytes(), name
    assert len(before["nodes"]) > 255 and len(before["lights"]) > 0
