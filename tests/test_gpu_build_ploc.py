"""The PLOC topology stage of the device builder (rodent_hip_build_bvh2_tri1_ploc, include/rodent_build.h; csrc/build_ploc.h) on the GPU.

* its nodes, triangles and info words equal tests/ploc_model.py's byte for byte: the Cornell box, seeded soups at the block, halo and
  finisher edges (radius 1, 8, 64, also beyond n; max_leaf 1, 4; 0 and 2 treelet passes), identical triangles, a split front, small
  depth limits, the atrium;
* the schedule (wide_iterations) changes no byte, also where the finisher starts with more clusters than it keeps in LDS;
* any stream, reused scratch and `out=` give the same bytes; a flagged mesh raises BuildError and the call returns;
* every order-preserving traversal variant on the PLOC trees reproduces the oracle bit for bit, and where the answers differ from the
  host SBVH's the ray is ambiguous;
* build_wide, the renderer's scene, `rodent --gpu-bvh --ploc-radius` and the gpubuild tool take the option.
Every tree is downloaded and checked on the host (trbvh_model.check_structure) before anything traces or renders it.
"""
import copy
import subprocess

import numpy as np
import pytest

import collapse_bounded_model as BM
import ploc_model as P
import split_model as SP
import trbvh_model as T
from conftest import GOLDEN, ambiguous_mask
from rodent_amd import scene as S
from test_gpu_build import FILM_ATOL, FILM_RTOL, atrium, cornell_scene, gb, soup  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
RADII = (1, 8, 64)
SIZES = (1, 2, 3, 17, 255, 256, 257, 1025, 3000)
_clusterings = {}


def cluster_once(leafbox, radius, depth_limit=0):
    """ploc_model.cluster, computed once per input: the clustering does not depend on max_leaf or the passes."""
    key = (leafbox.tobytes(), radius, depth_limit)
    if key not in _clusterings:
        _clusterings[key] = P.cluster(leafbox, radius, depth_limit)
    return _clusterings[key]


def model(v, ix, max_leaf, passes, radius, **kw):
    return P.build(v, ix, max_leaf, passes, radius, cluster_fn=cluster_once, **kw)


def checked(gb, bvh, num_tris, max_leaf, split=False):
    nodes, tris = gb.download(bvh)
    depth = (SP.check_split_structure(nodes, tris, num_tris, max_leaf, SP.MAX_PIECES) if split else
             T.check_structure(nodes, tris, num_tris, max_leaf))
    assert depth == bvh.depth == bvh.info[1] and len(nodes) == bvh.info[0] and len(tris) == bvh.info[4] == bvh.num_tris
    return nodes, tris


def assert_same_bytes(gb, bvh, want, num_tris, max_leaf, split=False):
    assert len(bvh.info) == 8 and np.array_equal(bvh.info, want[2]), (bvh.info, want[2])
    nodes, tris = checked(gb, bvh, num_tris, max_leaf, split)
    assert nodes.tobytes() == want[0].tobytes()
    assert tris.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("max_leaf, passes", [(1, 0), (4, 0), (1, 2), (4, 2)])
def test_bytes_equal_the_model_cornell_and_soups(gb, cornell_scene, max_leaf, passes, radius):
    cases = [("cornell", cornell_scene.vertices, cornell_scene.indices)]
    cases += [(f"soup{n}", *soup(n, n + 1)) for n in SIZES] + [("soup3000-flat", *soup(3000, 3))]
    for name, v, ix in cases:
        bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes, ploc_radius=radius)
        try:
            assert_same_bytes(gb, bvh, model(v, ix, max_leaf, passes, radius), len(ix), max_leaf)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("radius", RADII)
def test_identical_triangles(gb, radius):
    one = np.random.default_rng(1).uniform(-1, 1, (1, 9)).astype(np.float32)
    v = np.zeros((900, 4), np.float32)
    v[:, :3] = np.repeat(one, 300, 0).reshape(900, 3)
    ix = np.zeros((300, 4), np.int32)
    ix[:, :3] = np.arange(900).reshape(300, 3)
    bvh = gb.build_bvh2(v, ix, 1, ploc_radius=radius)
    assert_same_bytes(gb, bvh, model(v, ix, 1, 0, radius), 300, 1)
    assert bvh.depth <= P.clog2(300) + 1


def test_split_front(gb, cornell_scene):
    for v, ix in ((cornell_scene.vertices, cornell_scene.indices), soup(257, 6)):
        for max_leaf, passes in ((2, 0), (4, 2)):
            bvh = gb.build_bvh2(v, ix, max_leaf, treelet_passes=passes, split_budget=1.0, ploc_radius=8)
            assert bvh.num_tris > len(ix)
            assert_same_bytes(gb, bvh, model(v, ix, max_leaf, passes, 8, budget=1.0), len(ix), max_leaf, split=True)


@pytest.mark.parametrize("n", [64, 1000])
def test_depth_limits(gb, n):
    v, ix = soup(n, n)
    for extra in (0, 1, 3):
        D = P.clog2(n) + extra
        bvh = gb.build_bvh2(v, ix, 1, ploc_radius=8, depth_limit=D)
        assert_same_bytes(gb, bvh, model(v, ix, 1, 0, 8, depth_limit=D), n, 1)
        assert bvh.depth <= D
        if extra == 0:
            assert bvh.info[7] == P.nn_iterations(n) + P.clog2(n)
    free, same = gb.build_bvh2(v, ix, 1, ploc_radius=8), gb.build_bvh2(v, ix, 1, ploc_radius=8, depth_limit=56)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download(free), gb.download(same)))
    with pytest.raises(gb.BuildError):
        gb.build_bvh2(v, ix, 1, ploc_radius=8, depth_limit=P.clog2(n) - 1)
    with pytest.raises(gb.BuildError):
        gb.build_bvh2(v, ix, 1, ploc_radius=8, depth_limit=40, treelet_passes=1)


@pytest.fixture(scope="module")
def atrium_ploc(gb, atrium):
    """The atrium at radius 16 with 0 and 1 pass: the built trees, checked, and the model's."""
    out = {}
    for passes in (0, 1):
        bvh = gb.build_bvh2(atrium.vertices, atrium.indices, 2, treelet_passes=passes, ploc_radius=16)
        out[passes] = bvh, checked(gb, bvh, atrium.num_tris, 2), model(atrium.vertices, atrium.indices, 2, passes, 16)
    return out


@pytest.mark.parametrize("passes", [0, 1])
def test_bytes_equal_the_model_atrium(gb, atrium, atrium_ploc, passes):
    bvh, (nodes, tris), want = atrium_ploc[passes]
    assert np.array_equal(bvh.info, want[2]), (bvh.info, want[2])
    assert nodes.tobytes() == want[0].tobytes() and tris.tobytes() == want[1].tobytes()
    assert bvh.info[7] <= P.nn_iterations(atrium.num_tris)


def test_the_schedule_changes_no_byte(gb):
    v, ix = soup(3000, 3001)
    want = model(v, ix, 2, 1, 8)
    for wide in (0, 3, -1, 255):                         # 0: the finisher walks 3000 clusters in global memory before it keeps them in LDS
        bvh = gb.build_bvh2(v, ix, 2, treelet_passes=1, ploc_radius=8, wide_iterations=wide)
        assert_same_bytes(gb, bvh, want, len(ix), 2)


def test_deterministic_across_streams_and_reused_scratch(gb):
    import torch
    v, ix = soup(3000, 8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = gb.build_bvh2(v, ix, 2, stream=s1, ploc_radius=16, treelet_passes=1)
    b = gb.build_bvh2(v, ix, 2, stream=s2, ploc_radius=16, treelet_passes=1)
    ref = checked(gb, a, len(ix), 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(b))) and np.array_equal(a.info, b.info)
    big = gb.build_bvh2(*soup(20001, 3), 2, ploc_radius=16, treelet_passes=1)
    big.scratch.fill_(0xA5)
    c = gb.build_bvh2(v, ix, 2, scratch=big.scratch, out=big, ploc_radius=16, treelet_passes=1)
    assert c.scratch is big.scratch and c.nodes is big.nodes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, gb.download(c))) and np.array_equal(a.info, c.info)


def test_bad_index_and_nan_raise_device_flags(gb):
    v, ix = soup(1000, 4)
    bad, nan = ix.copy(), v.copy()
    bad[500, 1] = len(v)
    nan[1234, 1] = np.nan
    with pytest.raises(gb.BuildError, match="index.*non-finite"):
        gb.build_bvh2(nan, bad, ploc_radius=8, treelet_passes=1)
    assert gb.build_bvh2(v, ix, ploc_radius=8, treelet_passes=1).info[2] == 0


def rays_of(cornell, atrium_scene):
    from rodent_amd import formats as F
    from rodent_amd import raygen, scenes
    eye, d, up, fov = scenes.CAMERAS["atrium"]
    n4, _ = F.read_bvh(scenes.scene_bvh("atrium"), F.BVH4_TRI4)
    lo, hi = raygen.scene_bounds(n4)
    return {"cornell": list(cornell.ray_sets.values()),
            "atrium": [raygen.primary_rays(eye, d, up, fov, 64, 48, 0.0, scenes.PRIMARY_TMAX),
                       raygen.random_rays(lo, hi, 4096, 42, 0.0, scenes.RANDOM_TMAX)]}


@pytest.mark.parametrize("which", ["cornell", "atrium"])
def test_traversal_is_bit_exact_and_agrees_with_the_sbvh(gb, oracle, cornell, cornell_scene, atrium, atrium_ploc, which):
    from rodent_amd import abi
    sc = cornell_scene if which == "cornell" else atrium
    if which == "cornell":
        bvh = gb.build_bvh2(sc.vertices, sc.indices, 2, ploc_radius=16)
        nodes, tris = checked(gb, bvh, sc.num_tris, 2)
    else:
        bvh, (nodes, tris), _ = atrium_ploc[1]
    for rays in rays_of(cornell, atrium)[which]:
        for any_hit in (False, True):
            ref, st = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
            assert st["max_stack"] < 64
            for variant in abi.order_preserving_variants(2):
                got = abi.traverse(bvh, rays, any_hit=any_hit, variant=variant)
                bad = np.nonzero(got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4))[0]
                assert len(bad) == 0, f"{abi.variants(2)[variant]} any_hit={any_hit}: {len(bad)} rays differ"
        got = abi.traverse(bvh, rays, variant=0)
        sbvh, _ = oracle.traverse(2, sc.nodes, sc.tris, rays)
        diff = np.nonzero((got["tri_id"] != sbvh["tri_id"]) | (got["t"] != sbvh["t"]))[0]
        if len(diff):
            brute, second = oracle.brute_force(tris, rays[diff])
            amb = ambiguous_mask(brute, second)
            assert amb.all(), f"{(~amb).sum()} differing rays are not ambiguous, first {diff[~amb][0]}"


def test_wide_collapse_of_a_ploc_tree(gb):
    v, ix = soup(3000, 5)
    wide = gb.build_wide(v, ix, 8, ploc_radius=8, stack_limit=63)
    m_nodes, m_tris, _ = model(v, ix, 2, 0, 8)
    got2 = gb.download(wide.bvh2)
    assert got2[0].tobytes() == m_nodes.tobytes() and got2[1].tobytes() == m_tris.tobytes()
    want = BM.collapse(8, m_nodes, m_tris, 63)
    assert wide.info.tolist() == want[2].tolist() and wide.info[3] <= 63
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gb.download_wide(wide), want[:2]))


def test_renderer_scene_with_a_ploc_hierarchy(gb, oracle, cornell_scene):
    from rodent_amd import render as R
    sc = cornell_scene
    W, H, cam = 160, 120, S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, 160, 120)
    m_nodes, m_tris, _ = model(sc.vertices, sc.indices, 2, 0, 16)
    T.check_structure(m_nodes, m_tris, sc.num_tris, 2)
    r = R.Renderer(sc, W, H, 2, 6, gpu_bvh=2, gpu_bvh_ploc=16)
    got_nodes, got_tris = r.scene_bvh()
    assert got_nodes.tobytes() == m_nodes.tobytes() and got_tris.tobytes() == m_tris.tobytes()
    r.render(cam, 0)
    c = r.counters(); film_g = r.film(); r.close()
    built = copy.copy(sc)
    built.nodes, built.tris = got_nodes, got_tris
    film_o, counts = oracle.render(built, cam, 0, 2, 6, W, H)
    assert (c["primary_rays"], c["shadow_rays"]) == (counts[0], counts[1])
    assert np.allclose(film_g, film_o, rtol=FILM_RTOL, atol=FILM_ATOL) and film_g.mean() > 0.01
    with pytest.raises(ValueError, match="gpu_bvh"):
        R.Renderer(sc, 16, 16, gpu_bvh_ploc=16)


def test_rodent_cli_ploc_radius_matches_the_reference_image(gb, native_build, tmp_path):
    from PIL import Image
    out = tmp_path / "o.png"
    scene = ["--scene", GOLDEN / "cornell_box.obj"]
    cmd = [native_build.BIN_DIR / "rodent", *scene, "--gpu-bvh", "--ploc-radius", "16", "--treelet-passes", "1", "--bench", "50", "--eye",
           "0", "1", "2.7", "--dir", "0", "0", "-1", "--up", "0", "1", "0", "--width", "1080", "--height", "720", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = np.array(Image.open(out).convert("RGB")).astype(np.float32)
    ref = np.array(Image.open(GOLDEN / "ref-cornell.png").convert("RGB")).astype(np.float32)
    mse = ((img - ref) ** 2).mean() / 255.0 ** 2
    assert mse < 3e-4, mse
    for bad in (["--ploc-radius", "16"], ["--gpu-bvh", "--ploc-radius", "65"]):
        r = subprocess.run([native_build.BIN_DIR / "rodent", *scene, *bad, "--bench", "1"], capture_output=True, text=True)
        assert r.returncode != 0 and "--ploc-radius" in r.stdout + r.stderr


def test_gpubuild_tool_ploc_radius(gb, native_build, cornell_scene, tmp_path):
    import sys
    from rodent_amd import formats as F
    S.convert(GOLDEN / "cornell_box.obj", tmp_path / "c.rscene")
    out = tmp_path / "c.bvh"
    subprocess.run([sys.executable, "-m", "rodent_amd.gpubuild", tmp_path / "c.rscene", "-o", out, "--max-leaf", "4", "--ploc-radius", "8",
                    "--depth-limit", "20"], check=True, cwd=native_build.ROOT)
    nodes, tris = F.read_bvh(out, F.BVH2_TRI1)
    m_nodes, m_tris, _ = model(cornell_scene.vertices, cornell_scene.indices, 4, 0, 8, depth_limit=20)
    assert nodes.tobytes() == m_nodes.tobytes() and tris.tobytes() == m_tris.tobytes()
