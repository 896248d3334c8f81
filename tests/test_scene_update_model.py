"""tests/scene_update_model.py, the CPU model of the device scene update (rodent_hip_scene_refit_device), checked without a GPU.

* on the Cornell box (an OBJ without `vn` lines) it reproduces the loader's face normals, vertex normals and light records byte for byte;
* its level-by-level top image equals a plain sequential breadth-first walk on trees of 1, 30, 31, 32, 255, 256 and 999 nodes, among them
  a chain, a complete tree (a level of 128 nodes) and the max_leaf 1 LBVH of a 1000-triangle soup;
* the library exports the entries of the device path.
"""
import numpy as np
import pytest

import lbvh_model
import scene_update_model as M
from conftest import GOLDEN
from rodent_amd import formats as F
from rodent_amd import scene as S


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


def test_the_model_reproduces_the_loaders_tables_on_the_cornell_box(cornell_scene):
    sc = cornell_scene
    assert "\nvn " not in (GOLDEN / "cornell_box.obj").read_text()
    fn = M.face_normals(sc.vertices, sc.indices)
    normals = M.smooth_normals(fn, sc.indices, len(sc.vertices))
    # the light table from nothing but the colours: every light of the loader's is bound to a triangle
    blank = np.zeros_like(sc.lights)
    blank["color"] = sc.lights["color"]
    lights = M.light_records(blank, sc.vertices, sc.indices, sc.materials, sc.light_ids)
    for a in (fn, normals, lights["v0"], lights["v1"], lights["v2"], lights["n"], lights["inv_area"]):
        assert not np.isnan(a).any()
    assert len(sc.lights) > 0 and (M.light_triangles(sc.indices, sc.materials, sc.light_ids, len(sc.lights)) >= 0).all()
    assert fn.tobytes() == sc.face_normals.tobytes()
    assert normals.tobytes() == sc.normals.tobytes()
    assert lights.tobytes() == sc.lights.tobytes()
    shade = M.tri_shade(fn, normals, sc.indices)
    assert shade.shape == (sc.num_tris, 12) and shade[3, 3:6].tobytes() == sc.normals[sc.indices[3, 0], :3].tobytes()


def test_smooth_normals_order_valence_and_the_unused_vertex():
    v, ix, light_ids, lights = M.indexed_soup(257, 5)
    fn = M.face_normals(v, ix)
    assert not np.isnan(fn).any()
    first, tri = M.incidence(ix, len(v))
    assert first[1] - first[0] >= 70 and first[-1] - first[-2] == 0
    normals = M.smooth_normals(fn, ix, len(v))
    assert normals[-1].tolist() == [0, 1, 0, 0]                      # named by nobody
    for vertex in (0, 1, len(v) // 2):                               # the stated order, one addition at a time
        s = np.zeros(3, np.float32)
        for t in range(len(ix)):
            for k in range(3):
                if ix[t, k] == vertex:
                    s = s + fn[t, :3]
        l2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        want = s * (np.float32(1.0) / np.sqrt(l2)) if l2 > np.finfo(np.float32).eps else np.float32([0, 1, 0])
        assert normals[vertex, :3].tobytes() == want.astype(np.float32).tobytes()
    # a corner counted twice; a NaN sum falls back to (0, 1, 0)
    v2, ix2, *_ = M.indexed_soup(65, 7, twice=True)
    first2, tri2 = M.incidence(ix2, len(v2))
    assert (tri2[first2[ix2[1, 0]]: first2[ix2[1, 0] + 1]] == 1).sum() == 2
    fn2 = M.face_normals(v2, ix2)
    assert np.isnan(fn2[1, :3]).all() and np.isnan(fn2).sum() == 3
    assert M.smooth_normals(fn2, ix2, len(v2))[ix2[1, 0]].tolist() == [0, 1, 0, 0]
    # lights: the lowest emissive triangle wins, the light nobody names keeps its bytes
    moved = M.shear(v)
    out = M.light_records(lights, moved, ix, np.zeros(2, S.MATERIAL), light_ids)
    assert out.tobytes() == lights.tobytes()                         # no emissive material: nothing is bound
    mats = np.zeros(2, S.MATERIAL); mats["emissive"][1] = 1
    out = M.light_records(lights, moved, ix, mats, light_ids)
    assert out[-1].tobytes() == lights[-1].tobytes() and out["color"].tobytes() == lights["color"].tobytes()
    assert out["v0"][0, :3].tobytes() == moved[ix[0, 0], :3].tobytes() and (light_ids == 0).sum() > 2


def sequential_image(nodes, capacity):
    """The host's build_image(): a queue, one node at a time."""
    words = nodes.view(np.int32).reshape(-1, 16)
    image = np.zeros((capacity, 16), np.int32)
    slots = [1]
    k = 0
    while k < len(slots):
        rec = words[slots[k] - 1].copy()
        for j in range(2):
            c = int(rec[12 + j])
            if c > 0 and len(slots) < capacity:
                rec[12 + j] = M.LDS_TAG + len(slots) * 64
                slots.append(c)
        rec[14], rec[15] = slots[k], 0
        image[k] = rec
        k += 1
    return image


def random_tree(n, seed):
    """n inner nodes, each new one hung into a random open slot; node ids in no particular order; pad words non-zero."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros(n, F.NODE2)
    nodes["bounds"] = rng.uniform(-5, 5, (n, 12)).astype(np.float32)
    nodes["pad"] = 77
    ids = rng.permutation(np.arange(2, n + 1))
    open_slots = [(1, 0), (1, 1)]
    for c in ids:
        p, j = open_slots.pop(int(rng.integers(len(open_slots))))
        nodes["child"][p - 1, j] = c
        open_slots += [(int(c), 0), (int(c), 1)]
    for leaf, (p, j) in enumerate(open_slots):
        nodes["child"][p - 1, j] = ~leaf
    return nodes


def complete_tree(n, seed):
    nodes = random_tree(n, seed)
    for i in range(1, n + 1):
        nodes["child"][i - 1] = [2 * i if 2 * i <= n else ~(2 * i), 2 * i + 1 if 2 * i + 1 <= n else ~(2 * i + 1)]
    return nodes


def chain(n):
    from conftest import chain_bvh2
    return chain_bvh2(n)[0]


def tree_cases():
    single = np.zeros(1, F.NODE2); single["child"][0] = [~0, 0]
    v, ix, *_ = M.indexed_soup(1000, 11)
    soup_nodes = lbvh_model.build(v, ix, max_leaf=1)[0]
    assert len(soup_nodes) == 999
    cases = [("single", single), ("soup999", soup_nodes), ("chain32", chain(32)), ("chain256", chain(256)),
             ("complete255", complete_tree(255, 1)), ("complete256", complete_tree(256, 2))]
    cases += [(f"random{n}", random_tree(n, n)) for n in (30, 31, 32, 255, 256)]
    return cases


def test_top_image_equals_the_sequential_walk():
    widest = 0
    for name, nodes in tree_cases():
        for capacity in (31, 255):
            got, want = M.top_image(nodes, capacity), sequential_image(nodes, capacity)
            assert not np.isnan(got.view(np.float32)[:, :12]).any(), name
            assert got.tobytes() == want.tobytes(), (name, capacity)
            used = int((got[:, 14] > 0).sum())
            assert used == min(capacity, len(nodes)) and not got[used:].any(), (name, capacity)
        if name == "complete255":                                     # every level of it is in the large image: 1, 2, ... 128 nodes
            widest = 128
            assert (M.top_image(nodes, 255)[:, 12:14] < M.LDS_TAG).sum() == 256     # 128 leaves' two slots
    assert widest > 64


def test_the_library_exports_the_device_path(native_build):
    from rodent_amd import render
    l = render.lib()                                                  # loads without a GPU; a missing symbol raises AttributeError
    for name in ("rodent_hip_scene_refit_prepare", "rodent_hip_scene_refit_device", "rodent_hip_scene_refit_status",
                 "rodent_hip_scene_tables"):
        assert name in render.RENDER_EXPORTS and getattr(l, name) is not None, name
