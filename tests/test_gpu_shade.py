"""The shader (k_shade) and ray generation (k_generate) against the CPU oracle, vertex by vertex and word by word.

Kernels and oracle are compiled without contraction and written with the same explicit operations (rodent_amd/build.py), so the
bar is BIT EQUALITY of every word the stages write -- NaNs included -- and of everything they must leave alone.  Every comparison
is against oracle.binding.shade_vertices / emit_samples evaluated on the stream contents the GPU stage was actually given (read back
before the launch): nothing compounds across bounces and a traversal difference cannot pass for a shader difference.  The film gets
one float32 add per emitting vertex (1 spp: a pixel holds one vertex per bounce), so it is exact as well."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import shade_fixtures as SF
from conftest import GOLDEN
from rodent_amd import scene as S
from shade_fixtures import H, MAXLEN, W, assert_same, sentinel

pytestmark = pytest.mark.gpu
CAP = W * H                                                      # 6144 rays: the largest stream of this module


@pytest.fixture(scope="module")
def cornell_scene(native_build, tmp_path_factory):
    return S.convert(GOLDEN / "cornell_box.obj", tmp_path_factory.mktemp("scene") / "cornell.rscene")


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


@pytest.fixture()
def scenes(cornell_scene, materials_scene, textured_scene):
    return {"cornell": cornell_scene, "materials": materials_scene, "textured": textured_scene[0]}


def streams(R, cap):
    l = R.stage_lib()
    p, q, s = R.PrimaryStream(), R.PrimaryStream(), R.SecondaryStream()
    l.rodent_gpu_get_first_primary_stream(0, C.byref(p), cap)
    l.rodent_gpu_get_second_primary_stream(0, C.byref(q), cap)
    l.rodent_gpu_get_secondary_stream(0, C.byref(s), cap)
    assert SF.slab_cap(p) == SF.slab_cap(q) == SF.slab_cap(s) >= cap
    return l, p, q, s


@contextlib.contextmanager
def staged(R, scene, cap=CAP):
    """The scene on the device, a W x H film at 1 spp, and the three stream slabs."""
    r = R.Renderer(scene, W, H, 1, MAXLEN, mapping="streaming")
    try:
        yield (r,) + streams(R, cap)
    finally:
        r.close()


def assert_film(got, want, what):
    """Bit patterns; a NaN pixel (the sum's, not the shader's) has to be a NaN."""
    same = (SF.bits(got) == SF.bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {int((~same).sum())} film words differ, first at pixel {np.argwhere(~same)[0].tolist()}: " \
                       f"{got[~same][0]!r} against {want[~same][0]!r}"


# ---- a. ray generation ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(96, 64), (67, 5), (1, 1)])
def test_generated_rays_equal_the_oracle(R, oracle, w, h):
    """Every word of every generated entry: id = pixel, org = eye, dir and rnd = emit_samples as bytes, tmin 0, tmax FLT_MAX, mis 0,
    contrib 1, depth 0; hit records and the entries in front of and behind the appended range keep their 0xCDCDCDCD."""
    cam = SF.camera("cornell", w, h)
    st = R.make_settings(cam)
    for spp in (1, 3):
        total = w * h * spp
        l, p, q, s = streams(R, total + 64)
        for it in (0, 7):
            for size_before, first_ray in ((0, 0), (37, min(5, total - 1))):
                before = sentinel(p, SF.P_ROWS)
                SF.write_slab(R, p, before)
                p.size = size_before
                n = total - first_ray
                l.hip_generate_rays(0, C.byref(p), total + 64, first_ray, n, C.byref(st), it, w, h, 0, spp, None)
                assert p.size == size_before + n
                want = SF.generated_slab(cam, it, w, h, first_ray, n, 0, spp, before, size_before)
                assert (want[SF.ID, size_before:p.size].view("<i4") == (first_ray + np.arange(n)) // spp).all()
                assert_same(SF.read_slab(R, p, SF.P_ROWS), want, f"{w}x{h} spp {spp} iter {it} first ray {first_ray}")


# ---- b. natural vertices, shaded in place ------------------------------------------------------------
_natural_counts = {}


def run_natural(R, name, scene):
    cam = SF.camera(name)
    counts = {}
    with staged(R, scene) as (r, l, p, q, s):
        st = R.make_settings(cam)
        SF.write_slab(R, p, sentinel(p, SF.P_ROWS)); SF.write_slab(R, q, sentinel(q, SF.P_ROWS))
        p.size = 0
        l.hip_generate_rays(0, C.byref(p), CAP, 0, W * H, C.byref(st), 0, W, H, 0, 1, None)
        bounce = 0
        while p.size > 0:
            n = p.size
            l.hip_traverse_primary(0, C.byref(p), None)
            SF.write_slab(R, s, sentinel(s, SF.S_ROWS))
            p0, s0, film0 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS), SF.read_film(R)
            l.hip_shade(0, C.byref(p), C.byref(s), n, None)
            p1, s1, film1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS), SF.read_film(R)
            exp = SF.Expected(scene, p0, s0, n, MAXLEN)
            what = f"{name}, bounce {bounce}, {n} rays ({int(exp.live.sum())} hits)"
            assert_same(p1, exp.primary, what + ", primary stream")
            assert_same(s1, exp.secondary, what + ", secondary stream")
            assert_film(film1, exp.film_after(film0, 1.0), what)
            for k, c in SF.corpus_counts(scene, exp.vertices, exp.shade).items():
                counts[k] = counts.get(k, 0) + c
            alive = l.hip_compact_primary(0, C.byref(p), C.byref(q), None)
            assert alive == int(exp.bounce.sum()) == q.size
            p, q = q, p
            bounce += 1
        assert 2 <= bounce <= MAXLEN + 1
    _natural_counts[name] = counts
    return counts


@pytest.mark.parametrize("name", ["cornell", "materials", "textured"])
def test_natural_vertices_shade_bit_equal(R, oracle, scenes, name):
    """generate -> hip_traverse_primary -> read -> hip_shade -> read -> hip_compact_primary, every bounce until the stream is empty:
    both streams whole (entries that missed: both ids -1 and nothing else; sentinels intact) and the film, against the oracle."""
    run_natural(R, name, scenes[name])


def test_natural_corpus_is_not_vacuous(R, oracle, scenes):
    """The three scenes together shade every material class, emitters, textured materials, back-face hits and vertices at depth >= 3
    at least 50 times each (test_shade_oracle.py shows the same for the oracle alone)."""
    total = {}
    for name, scene in scenes.items():
        for k, c in (_natural_counts.get(name) or run_natural(R, name, scene)).items():
            total[k] = total.get(k, 0) + c
    assert set(total) == set(SF.CLASSES) | {"emitter", "textured", "leaving", "deep"}
    assert all(c >= 50 for c in total.values()), total


# ---- c. crafted vertices ------------------------------------------------------------------------------
REPLICATION = 24                                                 # random states per crafted vertex


@pytest.mark.parametrize("name", ["materials", "textured"])
def test_crafted_vertices_shade_bit_equal(R, oracle, scenes, name):
    """The edge cases of shade_fixtures.crafted_vertices through hip_shade: every word of both streams and the film, NaNs as bits.
    Vertices whose emits / shadow / bounce decision is an exact tie by construction stay in."""
    scene = scenes[name]
    v, groups = SF.crafted_vertices(scene, MAXLEN, REPLICATION, SF.texel_border_uvs(scene) if name == "textured" else ())
    n = len(v)
    assert 3000 < n <= CAP
    with staged(R, scene) as (r, l, p, q, s):
        p0, s0 = SF.slab_of(v, np.arange(n), scene, SF.slab_cap(p)), sentinel(s, SF.S_ROWS)
        SF.write_slab(R, p, p0); SF.write_slab(R, s, s0)
        film0 = SF.read_film(R)
        l.hip_shade(0, C.byref(p), C.byref(s), n, None)
        p1, s1, film1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS), SF.read_film(R)
    exp = SF.Expected(scene, p0, s0, n, MAXLEN)
    o = exp.shade
    assert exp.live.sum() == n and o["emits"].any() and o["shadow"].any() and o["bounce"].any() and not o["bounce"].all()
    bad = np.flatnonzero((p1 != exp.primary).any(0) | (s1 != exp.secondary).any(0))
    where = {g: int((groups[bad[bad < n]] == g).sum()) for g in np.unique(groups[bad[bad < n]])}
    assert_same(p1, exp.primary, f"{name}, primary stream, vertices that differ per group {where}")
    assert_same(s1, exp.secondary, f"{name}, secondary stream, vertices that differ per group {where}")
    assert_film(film1, exp.film_after(film0, 1.0), name)


# ---- d. stream sizes and the fused forms -----------------------------------------------------------------
def survivor_patterns(n, block, rng):
    """name -> mask over thread positions (which rays go on); patterns a size cannot hold are left out."""
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "random half": rng.random(n) < 0.5}
    last = np.zeros(n, bool); last[n - 1] = True
    out["last lane of the last wave"] = last
    if n > block:
        m = np.zeros(n, bool); m[block] = True
        out["lane 0 of block 1"] = m
    if n > 2 * block:
        m = np.ones(n, bool); m[block:2 * block] = False
        out["block 1 dead"] = m
    return out


@pytest.fixture(scope="module")
def bouncers(materials_scene):
    """Crafted vertices of the materials scene that go on at depth 1 by the oracle (and never at depth max_path_len)."""
    from oracle import binding as O
    v, _ = SF.crafted_vertices(materials_scene, MAXLEN, 2, seed=5)
    v["depth"] = 1
    return v[O.shade_vertices(materials_scene, v, MAXLEN)["bounce"] != 0]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_fused_compaction_slots(R, oracle, materials_scene, bouncers, block, mode):
    """hip_shade and hip_shade_compact at stream sizes around the wave and the workgroup, through no / the identity / the reversed / a
    random permutation, with survivor patterns that put the slot arithmetic (block total + earlier waves + lower lanes) on its edges.
    hip_shade in place equals the oracle; mode 1's `to` is exactly the stable compaction of that, mode 2's the same records in any
    block order; the returned size is the survivor count; shadow rays sit at index i; `to` behind the size, `to`'s hit records and
    `from` are untouched."""
    import torch
    scene = materials_scene
    rng = np.random.default_rng(block + mode)
    keys = (SF.ID, SF.RND)
    with staged(R, scene, 2 * 1024 + 32) as (r, l, p, q, s):
        cap = SF.slab_cap(p)
        for n in (1, 63, 64, 65, block - 1, block, block + 1, 2 * block + 1):
            for pattern, mask in survivor_patterns(n, block, rng).items():
                what = f"block {block}, mode {mode}, {n} rays, {pattern}"
                v = bouncers[(np.arange(n) * 7 + n) % len(bouncers)].copy()
                v["depth"] = np.where(mask, 1, MAXLEN)
                ids = (np.arange(n) * 5 + 3) % CAP                            # distinct pixels, not in stream order
                g0 = SF.slab_of(v, ids, scene, cap)
                dead = np.flatnonzero(~mask)
                SF.mark_missed(g0, dead[::5], scene)
                s0, q0 = sentinel(s, SF.S_ROWS), sentinel(q, SF.P_ROWS)
                # in place, on the stream in thread order
                SF.write_slab(R, p, g0); SF.write_slab(R, s, s0)
                l.hip_shade(0, C.byref(p), C.byref(s), n, None)
                p1, s1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
                exp = SF.Expected(scene, g0, s0, n, MAXLEN)
                assert np.array_equal(exp.bounce[:n], mask), what
                assert_same(p1, exp.primary, what + ", hip_shade primary")
                assert_same(s1, exp.secondary, what + ", hip_shade secondary")
                want_q, survivors = SF.compacted(p1, q0, p1[SF.ID].view("<i4")[:n] >= 0)
                assert survivors == int(mask.sum())
                for perm_name, perm in (("no", None), ("identity", np.arange(n)), ("reversed", np.arange(n)[::-1]),
                        ("random", rng.permutation(n))):
                    f0 = g0.copy()
                    if perm is not None:
                        f0[:, perm] = g0[:, :n]                               # thread i shades ray perm[i]
                        d_perm = torch.from_numpy(np.ascontiguousarray(perm, "<i4")).cuda()
                    SF.write_slab(R, p, f0); SF.write_slab(R, q, q0); SF.write_slab(R, s, s0)
                    torch.cuda.synchronize()
                    got = l.hip_shade_compact(0, C.byref(p), C.byref(q), C.byref(s), None if perm is None else d_perm.data_ptr(), n, mode,
                        block, None)
                    pf, qf, sf = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, q, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
                    at = f"{what}, {perm_name} permutation"
                    assert got == survivors == q.size, at
                    assert_same(pf, f0, at + ", `from`")
                    assert_same(sf, s1, at + ", secondary stream")
                    if mode == 2:                                             # blocks arrive in any order: the same records
                        order = lambda a: a[:, np.lexsort([a[k, :got] for k in reversed(keys)])]
                        assert_same(qf[:, got:], want_q[:, got:], at + ", `to` behind the new size")
                        assert_same(order(qf[:, :got]), order(want_q[:, :got]), at + ", `to` as a multiset")
                    else:
                        assert_same(qf, want_q, at + ", `to`")


def window_patterns(n, block):
    """name -> survivor mask over thread positions, by workgroup: what the look-back scan reads are the workgroups' totals."""
    group = np.arange(n) // block
    last = np.zeros(n, bool); last[n - 1] = True
    return {"everyone": np.ones(n, bool), "nobody in blocks 0 ... 63, everyone after": group >= 64, "only block 0": group == 0,
            "every other block empty": group % 2 == 0, "one survivor in the very last ray": last}


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_compaction_slots_past_one_window(R, oracle, materials_scene, bouncers, mode):
    """test_fused_compaction_slots with more workgroups than the 64 predecessors one round of the look-back scan reads: 64, 66 and 130
    workgroups of 256, so that the scan walks one full window, one window and a lane, two windows and a lane -- over totals that are all
    non-zero, all zero for a whole window (the walk has to go on behind them), zero from block 1 on, alternating, and zero but for the
    last ray.  The same assertions; no and a random permutation."""
    import torch
    scene, block = materials_scene, 256
    rng = np.random.default_rng(mode)
    with staged(R, scene, 129 * block + 5 + 32) as (r, l, p, q, s):
        cap = SF.slab_cap(p)
        for n in (64 * block, 65 * block + 1, 129 * block + 5):
            for pattern, mask in window_patterns(n, block).items():
                what = f"block {block}, mode {mode}, {n} rays, {pattern}"
                v = bouncers[(np.arange(n) * 7 + n) % len(bouncers)].copy()
                v["depth"] = np.where(mask, 1, MAXLEN)
                ids = (np.arange(n) * 5 + 3) % CAP                            # pixels of the film, not in stream order
                g0 = SF.slab_of(v, ids, scene, cap)
                dead = np.flatnonzero(~mask)
                SF.mark_missed(g0, dead[::5], scene)
                s0, q0 = sentinel(s, SF.S_ROWS), sentinel(q, SF.P_ROWS)
                SF.write_slab(R, p, g0); SF.write_slab(R, s, s0)
                l.hip_shade(0, C.byref(p), C.byref(s), n, None)
                p1, s1 = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
                exp = SF.Expected(scene, g0, s0, n, MAXLEN)
                assert np.array_equal(exp.bounce[:n], mask), what
                assert_same(p1, exp.primary, what + ", hip_shade primary")
                assert_same(s1, exp.secondary, what + ", hip_shade secondary")
                want_q, survivors = SF.compacted(p1, q0, p1[SF.ID].view("<i4")[:n] >= 0)
                assert survivors == int(mask.sum())
                for perm_name, perm in (("no", None), ("random", rng.permutation(n))):
                    f0 = g0.copy()
                    if perm is not None:
                        f0[:, perm] = g0[:, :n]                               # thread i shades ray perm[i]
                        d_perm = torch.from_numpy(np.ascontiguousarray(perm, "<i4")).cuda()
                    SF.write_slab(R, p, f0); SF.write_slab(R, q, q0); SF.write_slab(R, s, s0)
                    torch.cuda.synchronize()
                    got = l.hip_shade_compact(0, C.byref(p), C.byref(q), C.byref(s), None if perm is None else d_perm.data_ptr(), n, mode,
                        block, None)
                    pf, qf, sf = SF.read_slab(R, p, SF.P_ROWS), SF.read_slab(R, q, SF.P_ROWS), SF.read_slab(R, s, SF.S_ROWS)
                    at = f"{what}, {perm_name} permutation"
                    assert got == survivors == q.size, at
                    assert_same(pf, f0, at + ", `from`")
                    assert_same(sf, s1, at + ", secondary stream")
                    if mode == 2:                                             # blocks arrive in any order: the same records
                        # (pixels and vertices repeat at these sizes: ordered by every row, so that equal keys cannot hide a difference)
                        order = lambda a: a[:, np.lexsort(a[::-1, :got])]
                        assert_same(qf[:, got:], want_q[:, got:], at + ", `to` behind the new size")
                        assert_same(order(qf[:, :got]), order(want_q[:, :got]), at + ", `to` as a multiset")
                    else:
                        assert_same(qf, want_q, at + ", `to`")


def test_emissions_of_one_wave_on_one_pixel(R, oracle, materials_scene):
    """64 emitter hits of one pixel in one wave (summed across the lanes before the atomic): the pixel is the float64 sum of the oracle's
    emissions within 64 * 2^-24 of the summed magnitudes, the bound for 64 float32 additions in any order; no other pixel moves."""
    scene = materials_scene
    lamp = int(np.flatnonzero(scene.materials["emissive"][scene.indices[:, 3]] != 0)[0])
    v, g = SF.crafted_vertices(scene, MAXLEN, 64, seed=9)
    v = v[(v["prim"] == lamp) & (g == "depth")][:64].copy()
    rng = np.random.default_rng(3)
    v["contrib"] = rng.uniform(0.05, 1.0, (64, 3)); v["mis"] = rng.uniform(0.0, 4.0, 64)
    pixel = 1234
    with staged(R, scene) as (r, l, p, q, s):
        SF.write_slab(R, p, SF.slab_of(v, np.full(64, pixel), scene, SF.slab_cap(p))); SF.write_slab(R, s, sentinel(s, SF.S_ROWS))
        r.clear()
        l.hip_shade(0, C.byref(p), C.byref(s), 64, None)
        film = SF.read_film(R)
    o = oracle.shade_vertices(scene, v, MAXLEN)
    assert o["emits"].all() and (o["emitted"] > 0).all() and len(np.unique(o["emitted"][:, 0])) > 32
    e = o["emitted"].astype(np.float64)
    assert (np.abs(film[pixel] - e.sum(0)) <= 64 * 2.0 ** -24 * np.abs(e).sum(0)).all(), (film[pixel], e.sum(0))
    film[pixel] = 0
    assert not film.any()
