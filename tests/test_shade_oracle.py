"""CPU tests of the per-vertex oracle bindings (oracle.binding.shade_vertices / emit_samples): the reference every word of
tests/test_gpu_shade.py is compared with.  The bindings are pinned against oracle_render (a path walked in Python gives its film
byte for byte) and against float64 properties of the outputs; the corpus the GPU test relies on is shown not to be vacuous."""
import numpy as np
import pytest

import shade_fixtures as SF
from conftest import GOLDEN
from rodent_amd import scene as S

from shade_fixtures import W, H, MAXLEN, camera


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


@pytest.fixture(scope="module")
def corpora(oracle, cornell_scene, materials_scene, textured_scene):
    """Per scene: (scene, vertices, shade records) of every vertex the oracle shades at 96 x 64, 1 spp, max_path_len 6."""
    out = {}
    for name, sc in (("cornell", cornell_scene), ("materials", materials_scene), ("textured", textured_scene[0])):
        vs, os_ = [], []
        SF.walk_paths(sc, camera(name), 0, 1, MAXLEN, W, H, on_bounce=lambda b, v, o: (vs.append(v.copy()), os_.append(o.copy())))
        out[name] = (sc, np.concatenate(vs), np.concatenate(os_))
    return out


def test_dtypes_mirror_the_c_structs(oracle):
    l = oracle.lib()
    oracle.shade_vertices                                       # the bindings exist ...
    l.oracle_render_abi_sizes.restype = np.ctypeslib.ctypes.c_uint32
    sizes = [l.oracle_render_abi_sizes(k) for k in range(5)]
    assert sizes == [oracle.ORACLE_VERTEX.itemsize, oracle.ORACLE_SHADE.itemsize, 56, S.MATERIAL.itemsize, S.LIGHT.itemsize]
    assert sizes[:2] == [64, 104]                               # ... and are 16 / 26 words without padding
    assert oracle.ORACLE_SHADE.fields["rnd"][1] == 96 and oracle.ORACLE_VERTEX.fields["depth"][1] == 60


def test_walked_paths_reproduce_oracle_render(oracle, cornell_scene):
    """emit_samples + traverse + shade_vertices, additions in oracle_render's order: its film, byte for byte."""
    w, h, spp, maxlen = 32, 24, 2, 5
    cam = camera("cornell", w, h)
    for it in (0, 3):
        ref, _ = oracle.render(cornell_scene, cam, it, spp, maxlen, w, h, threads=1)
        film = SF.walk_paths(cornell_scene, cam, it, spp, maxlen, w, h)
        assert ref.mean() > 0.02
        assert film.tobytes() == ref.tobytes()


def test_emit_samples_is_the_seed_and_the_camera_ray(oracle):
    cam = camera("cornell", 67, 5)
    rnd, d = oracle.emit_samples(cam, 7, 67, 5, [0, 66, 13], [0, 4, 2], [0, 2, 1])
    for k, (x, y, s) in enumerate(((0, 0, 0), (66, 4, 2), (13, 2, 1))):
        seed = np.uint32(oracle.lib().oracle_seed(s, 7, x, y) & 0xFFFFFFFF)
        assert rnd[k] == xorshift(xorshift(np.array([seed])))[0]          # two randf draws: the pixel jitter
    n = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    assert np.abs(n - 1).max() <= 4 * 2.0 ** -23
    assert d[0, 0] < 0 < d[1, 0] and d[0, 1] > 0 > d[1, 1] and (d[:, 2] < 0).all()      # left / right, top / bottom of the image


def xorshift(x):
    x = np.where(x == 0, np.uint32(1), x).astype(np.uint32)
    x ^= x << np.uint32(13); x ^= x >> np.uint32(17); x ^= x << np.uint32(5)
    return x


def test_corpus_is_not_vacuous(corpora):
    """What test_gpu_shade.py asserts about its natural vertices holds for the oracle alone: every material class, emitters,
    textured materials, back-face hits and deep vertices are each shaded at least 50 times."""
    total = {}
    for name, (sc, v, o) in corpora.items():
        for k, c in SF.corpus_counts(sc, v, o).items():
            total[k] = total.get(k, 0) + c
    print(total)
    assert all(c >= 50 for c in total.values()), total
    assert set(total) == set(SF.CLASSES) | {"emitter", "textured", "leaving", "deep"}


def test_shade_vertices_properties(corpora):
    """float64 checks of shade_vertices on the materials scene's vertices: the shadow ray ends on a light, the continuation is a unit
    vector on the side of the surface its BSDF allows, the diffuse throughput is contrib * kd / rr, and the random state advances
    by the number of xorshift steps of the vertex's material class."""
    sc, v, o = corpora["materials"]
    f8 = np.float64
    mat = sc.materials[sc.indices[v["prim"], 3]]
    fn = sc.face_normals[v["prim"], :3].astype(f8)
    entering = (v["dir"].astype(f8) * fn).sum(1) <= 0
    side = np.where(entering[:, None], fn, -fn)

    # shadow rays: s_org + s_dir is a point of some light triangle.  s_dir = pos - point in float32 and coordinates are below 4:
    # a handful of roundings of 2^-24 * 4 each
    tol = 16 * 2.0 ** -24 * 4
    sh = o["shadow"] != 0
    assert sh.sum() > 1000
    pos = o["s_org"][sh].astype(f8) + o["s_dir"][sh].astype(f8)
    on_some = np.zeros(len(pos), bool)
    for L in sc.lights:
        a, b, c, n = (L[k][:3].astype(f8) for k in ("v0", "v1", "v2", "n"))
        in_plane = np.abs((pos - a) @ n) <= tol
        m = np.stack([b - a, c - a], 1)                                   # barycentrics by least squares
        uv, *_ = np.linalg.lstsq(m, (pos - a).T, rcond=None)
        inside = (uv[0] >= -tol) & (uv[1] >= -tol) & (uv[0] + uv[1] <= 1 + tol)
        on_some |= in_plane & inside
    assert on_some.all()

    # continuation rays
    b = o["bounce"] != 0
    assert b.sum() > 1000
    bd = o["b_dir"][b].astype(f8)
    # |b_dir| = 1 within 4 ulp of 1.0 (2^-23 each) PER SHADING STEP: black hands the incoming direction on, mirror / Phong / glass build
    # theirs from it as if it were a unit vector, so what |dir| itself is off by comes on top -- times k^2 = Ni^2 = 2.25 at most for a
    # refraction (|t|^2 = 1 + k^2 (|dir|^2 - 1)); only the diffuse lobe starts afresh from the shading normal
    din = v["dir"][b].astype(f8)
    carried = np.abs(np.sqrt((din * din).sum(1)) - 1) * np.select([mat["type"][b] == 1, mat["type"][b] == 5], [0.0, 2.25], 1.0)
    assert (np.abs(np.sqrt((bd * bd).sum(1)) - 1) <= 4 * 2.0 ** -23 + carried).all()
    lum2 = SF.f32(2) * ((v["contrib"][:, 0] * SF.f32(0.2126) + v["contrib"][:, 1] * SF.f32(0.7152)) + v["contrib"][:, 2] * SF.f32(0.0722))
    rr = np.minimum(lum2, SF.f32(0.75)).astype(f8)[b]
    cin, cout = v["contrib"][b].astype(f8), o["contrib"][b].astype(f8)
    facing = (bd * side[b]).sum(1)
    carries = (cout != 0).any(1)
    t = mat["type"][b]
    assert (facing[carries & (t != 5)] > 0).all()                          # reflection: the side the ray came from
    glass = carries & (t == 5)
    assert (glass & (facing < 0)).sum() > 20 and (glass & (facing > 0)).sum() > 5
    for sel, colour in ((glass & (facing < 0), "tf"), (glass & (facing > 0), "ks"), (carries & (t == 4), "ks"), (carries & (t == 1), "kd")):
        # seven roundings of 2^-24 at most between the float64 product and the shader's float32 chain
        want = cin[sel] * mat[colour][b][sel].astype(f8) / rr[sel, None]
        assert sel.sum() > 20 and np.abs(cout[sel] - want).max() <= 1e-6 * np.abs(want).max(), colour
    assert not carries[t == 0].any()                                       # black: nothing goes on

    # random states: light pick + two light coordinates (non-specular), the roulette, then the BSDF's own draws
    steps = {0: 4, 1: 6, 2: 6, 3: 7, 4: 1}
    for k, n in steps.items():
        sel = b & (mat["type"] == k)
        x = v["rnd"][sel].copy()
        for _ in range(n):
            x = xorshift(x)
        assert sel.sum() > 0 and np.array_equal(x, o["rnd"][sel]), k
    sel = b & (mat["type"] == 5)                                           # glass: one more draw unless totally reflected
    x1 = xorshift(v["rnd"][sel]); x2 = xorshift(x1)
    assert ((o["rnd"][sel] == x1) | (o["rnd"][sel] == x2)).all() and (o["rnd"][sel] == x1).any() and (o["rnd"][sel] == x2).any()
    # a vertex that does not bounce reports nothing
    assert not o["rnd"][~b].any() and not o["contrib"][~b].any()


def test_crafted_vertices_reach_their_edges(oracle, materials_scene, textured_scene):
    """The crafted set of test_gpu_shade.py, judged by the oracle: the depth group stops exactly at max_path_len, zero throughput
    never bounces, both sides of total internal reflection occur, nothing above the lamp is lit, and the groups are all there."""
    for sc, extra in ((materials_scene, ()), (textured_scene[0], SF.texel_border_uvs(textured_scene[0]))):
        v, g = SF.crafted_vertices(sc, MAXLEN, 8, extra)
        o = oracle.shade_vertices(sc, v, MAXLEN)
        assert {"depth", "contrib0", "rr_clamp", "rnd", "mis", "t", "uv", "backface", "grazing", "above_lamp"} <= set(g)
        d = g == "depth"
        assert not o["bounce"][d & (v["depth"] >= MAXLEN)].any() and o["bounce"][d & (v["depth"] < MAXLEN)].any()
        assert not o["bounce"][g == "contrib0"].any()
        assert not o["shadow"][g == "above_lamp"].any()
        assert not o["emits"][g == "backface"].any()
        assert o["emits"][g == "uv"].any()
        if (sc.materials["type"] == 5).any():
            gi = g == "glass_inside"
            tf = sc.materials["tf"][sc.materials["type"] == 5][0]
            fn = sc.face_normals[v["prim"][gi], :3]
            assert ((v["dir"][gi] * fn).sum(1) > 0).all()                   # back-face hits: the ray leaves the glass
            through = (o["bounce"][gi] != 0) & (np.abs(o["contrib"][gi] / v["contrib"][gi] * 0.75 - tf) < 1e-4).all(1)
            deg = np.repeat(SF.GLASS_DEGREES, 8)
            assert through[deg < 41.81].any() and not through[deg > 41.81].any() and o["bounce"][gi][deg > 41.81].any()
