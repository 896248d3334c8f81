"""The renderer's stream traversal kernels (rodent_amd/csrc/render_trace.h) against the oracle, ray by ray.

Rays from tests/stream_trace_fixtures.py go into the library's own streams; every route through launch_trace -- the one-chunk kernels with
k_trace_deep behind them, k_trace_persist<0|1|2>, k_trace_refill with and without closest-hit lanes, the fall-back for streams that are no
slabs -- is asserted BY KERNEL NAME (rodent_hip_render_trace_kernel_name) and compared:
* closest-hit pass: the five hit arrays (or the 20-byte records) byte for byte with stream_trace_fixtures.expected_records, ray i's record
  at index i, nothing written behind the last ray;
* shadow pass: spp = 1 and one pixel per live ray, so the film equals expected_film exactly; the counters grow by the rays traced.
Every route runs twice in a row (tickets, deep counts and the slot word are reset by the launch before) and is followed by another route.

What the module was seen to catch, each change made alone in render_trace.h and undone again:
* the lazy miss record storing the lane's canonical tmax: test_both_passes_in_one_launch[cornell|soup|padded] and the two shadow-order
  children fail -- 96 records of a specials set differ in `t`, 0x7FE00001 stored for the signalling NaN 0x7FA00001 (a denormal tmax comes
  through unchanged);
* `c0first` negated for k_trace_refill's closest-hit lanes: test_both_passes_in_one_launch on all three classes and the lane-refill cases of
  test_list_sizes_around_a_wave_and_a_ticket_group fail -- 208 records of the soup's segments and two of the Cornell edge rays name another
  triangle at the same t (the soup's triangles that lie three to a place; shared edges);
* `i <= ns` for `i < ns` in k_trace_persist's shadow branch: test_dead_shadow_rays_and_a_size_on_the_device[persist<1>] and [persist<2>]
  fail on the counter (1784 shadow rays counted for 1783).
k_trace_refill without its stack_reload was not run: the lane would go on with the spill mark as a node id and a cursor below its column,
and fetch from wherever that leads.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import stream_trace_fixtures as X                                # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0x7B7B7B7B
FILM_W = 512
CLASSES = ("cornell", "soup", "padded")


class Rig:
    """One hierarchy as the scene of device 0, a film of at least `pixels` pixels (spp 1), one primary and one secondary stream of the
    library for up to `capacity` rays."""

    def __init__(self, R, oracle, h, capacity=4096, pixels=4096):
        self.R, self.oracle, self.h = R, oracle, h
        self.pixels = pixels
        self.r = R.Renderer(h.scene, FILM_W, (pixels + FILM_W - 1) // FILM_W, spp=1, max_path_len=4)
        self.l = R.stage_lib()
        self.p, self.s = R.PrimaryStream(), R.SecondaryStream()
        self.l.rodent_gpu_get_first_primary_stream(0, C.byref(self.p), capacity)
        self.l.rodent_gpu_get_secondary_stream(0, C.byref(self.s), capacity)
        self.cap = (capacity & ~31) + 32
        self.expect = {}                                         # id(rays) -> expected records
        self.keep = []

    def close(self):
        self.r.close()

    # ---- options -------------------------------------------------------------------------------------------------------------------
    def configure(self, lds_image=1, persistent=0, refill=(0, 0), min_rays=-1):
        l = self.l
        l.rodent_hip_render_lds_image(0, lds_image); l.rodent_hip_render_trace_persistent(0, persistent)
        l.rodent_hip_render_trace_refill(0, *refill); l.rodent_hip_render_persist_min_rays(0, min_rays)

    def kernel(self):
        return self.r.trace_kernel_name()

    # ---- streams -------------------------------------------------------------------------------------------------------------------
    def write_rays(self, stream_rays, rays, ids):
        W = self.R.write_stream_array
        W(stream_rays.id, np.asarray(ids, "<i4"))
        for k, name in enumerate(("org_x", "org_y", "org_z")):
            W(getattr(stream_rays, name), rays["org"][:, k])
        for k, name in enumerate(("dir_x", "dir_y", "dir_z")):
            W(getattr(stream_rays, name), rays["dir"][:, k])
        W(stream_rays.tmin, rays["tmin"]); W(stream_rays.tmax, rays["tmax"])

    def load_primary(self, rays):
        self.write_rays(self.p.rays, rays, np.arange(len(rays)))
        self.p.size = len(rays)

    def load_shadow(self, rays, ids, colours):
        self.write_rays(self.s.rays, rays, ids)
        for k, name in enumerate(("color_r", "color_g", "color_b")):
            self.R.write_stream_array(getattr(self.s, name), colours[:, k])
        self.s.size = len(rays)

    def records(self, rays):
        key = id(rays)
        if key not in self.expect:
            self.keep.append(rays)
            self.expect[key] = X.expected_records(self.oracle, self.h.scene, rays)
        return self.expect[key]

    # ---- one closest-hit launch and its comparison ------------------------------------------------------------------------------------
    def check_primary(self, rays, launch, kernel, aos=False, moved=None, what=""):
        """`launch()` traces the n rays loaded into self.p; the record memory is poisoned first and compared afterwards as a whole:
        the records bit for bit, and the poison untouched behind them."""
        n, cap = len(rays), self.cap
        R = self.R
        R.write_stream_array(self.p.geom_id, np.full(5 * cap, POISON, "<u4"))
        for ptr in (moved or {}).values():
            R.write_stream_array(ptr, np.full(cap, POISON, "<u4"))
        before = self.r.counters()["primary_rays"]
        launch()
        assert self.kernel() == kernel, (what, self.kernel(), kernel)
        region = R.read_stream_array(self.p.geom_id, 5 * cap, "<u4")
        want = [np.ascontiguousarray(a).view("<u4") for a in self.records(rays)]
        if aos:
            got, exp = region[:5 * n].reshape(n, 5), np.stack(want, 1)
            bad = np.flatnonzero((got != exp).any(1))
            assert len(bad) == 0, (what, "records differ", len(bad), bad[:8], got[bad[:4]], exp[bad[:4]], rays[bad[:4]])
            assert (region[5 * n:] == POISON).all(), (what, "wrote behind the last record")
        else:
            arrays = region.reshape(5, cap).copy()
            for k, name in enumerate(("geom_id", "prim_id", "t", "u", "v")):
                if moved and name in moved:
                    assert (arrays[k] == POISON).all(), (what, name, "written in its old place")
                    arrays[k] = R.read_stream_array(moved[name], cap, "<u4")
                bad = np.flatnonzero(arrays[k, :n] != want[k])
                assert len(bad) == 0, (what, name, len(bad), bad[:8], arrays[k, bad[:8]], want[k][bad[:8]], rays[bad[:4]])
                assert (arrays[k, n:] == POISON).all(), (what, name, "wrote behind the last ray")
        assert self.r.counters()["primary_rays"] - before == n, what

    # ---- one shadow launch and its comparison -----------------------------------------------------------------------------------------
    def film_of(self, rays, ids, colours, size):
        key = (id(rays), id(ids), size)
        if key not in self.expect:
            self.keep += [rays, ids]
            self.expect[key] = X.expected_film(self.oracle, self.h.scene, rays, ids, colours, 1.0, size, self.pixels).astype("<f4")
        return self.expect[key]

    def check_shadow(self, rays, ids, colours, launch, kernel, size=None, what=""):
        """`launch()` traces the shadow rays loaded into self.s (the first `size` of them): one pixel per live ray, so the film is exact."""
        size = len(rays) if size is None else size
        self.r.clear()
        before = self.r.counters()["shadow_rays"]
        launch()
        assert self.kernel() == kernel, (what, self.kernel(), kernel)
        film = self.r.film().reshape(-1, 3)
        want = self.film_of(rays, ids, colours, size)
        bad = np.flatnonzero((film[:self.pixels] != want).any(1))
        assert len(bad) == 0, (what, "film differs", len(bad), bad[:8], film[bad[:4]], want[bad[:4]])
        assert not film[self.pixels:].any(), what
        assert self.r.counters()["shadow_rays"] - before == int((np.asarray(ids)[:size] >= 0).sum()), what

    # ---- entry points -----------------------------------------------------------------------------------------------------------------
    def primary_entry(self):
        self.l.hip_traverse_primary(0, C.byref(self.p), None)

    def secondary_entry(self):
        self.l.hip_traverse_secondary(0, C.byref(self.s), None)

    def streams(self, primary=True, coherent_from=0, shadow=True, size_dev=None, flags=0, expect_status=0):
        status = self.l.hip_traverse_streams(0, C.byref(self.p) if primary else None, coherent_from, C.byref(self.s) if shadow else None,
                                             C.c_void_p(size_dev.data_ptr()) if size_dev is not None else None, flags, None)
        assert status == expect_status, (status, expect_status)


def colours_for(n, seed=1):
    return np.random.default_rng(seed).uniform(0.1, 1.0, (n, 3)).astype("<f4")


@pytest.fixture()
def R(native_build):
    import torch
    from rodent_amd import render
    assert torch.cuda.is_available()
    return render


@pytest.fixture()
def rig_for(R, oracle):
    made = []

    def make(name, **kw):
        made.append(Rig(R, oracle, X.hierarchy(name, oracle), **kw))
        return made[-1]
    yield make
    for rig in made:
        rig.close()


REFILL = "k_trace_refill<1,true>"                                 # the default shadow order and miss record


@pytest.mark.parametrize("name", X.HIERARCHIES)
def test_lone_passes_on_every_kernel(rig_for, name):
    """hip_traverse_primary / hip_traverse_secondary through the one-chunk kernels with and without the LDS image (k_trace_deep picks up
    what outgrows their window), the whole-chunk persistent kernels, and the lane refill (shadow lanes only: a lone closest-hit pass of
    unknown coherence takes whole chunks)."""
    rig = rig_for(name)
    routes = [(dict(lds_image=1), "k_trace_primary<2,31>", "k_trace_secondary<2,31>"),
              (dict(lds_image=0), "k_trace_primary<1,0>", "k_trace_secondary<1,0>"),
              (dict(persistent=1, min_rays=0), "k_trace_persist<0>", "k_trace_persist<1>")]
    routes += [(dict(persistent=1, min_rays=0, refill=t), "k_trace_persist<0>", REFILL) for t in ((32, 32), (1, 1), (64, 64))]
    for set_name, rays in rig.h.ray_sets.items():
        n = len(rays)
        ids, colours = X.dead_ray_ids(n), colours_for(n)
        rig.load_primary(rays); rig.load_shadow(rays, ids, colours)
        for options, closest, shadow in routes:
            rig.configure(**options)
            for rep in range(2):
                what = (name, set_name, options, rep)
                rig.check_primary(rays, rig.primary_entry, closest, what=what)
                rig.check_shadow(rays, ids, colours, rig.secondary_entry, shadow, what=what)


@pytest.mark.parametrize("name", X.HIERARCHIES)
def test_both_passes_in_one_launch(rig_for, name):
    """hip_traverse_streams: k_trace_persist<2>, and k_trace_refill with closest-hit lanes at three pairs of thresholds, with the coherent
    part of the closest-hit list starting at 0, at an odd index near the middle and at n (nothing coherent), both passes or the closest-hit
    pass alone, five arrays or 20-byte records.  The closest-hit list ends inside a wave next to a non-empty shadow list (the shadow rays'
    indices start at the next whole chunk).  Records depend on none of this."""
    rig = rig_for(name)
    for set_name, rays in rig.h.ray_sets.items():
        n_s = len(rays)
        n = n_s if n_s % 64 else n_s - 37
        first = np.ascontiguousarray(rays[:n])
        ids, colours = X.dead_ray_ids(n_s), colours_for(n_s)
        rig.load_primary(first); rig.load_shadow(rays, ids, colours)
        mid = (n // 2) | 1
        cases = []
        for aos in (0, 1):
            cases.append((dict(refill=(0, 0)), True, 0, aos, "k_trace_persist<2>"))
        for t in ((40, 40), (1, 1), (64, 32)):
            cases += [(dict(refill=t), True, 0, 0, REFILL), (dict(refill=t), True, mid, 1, REFILL), (dict(refill=t), True, n, 0, REFILL),
                      (dict(refill=t, persistent=1, min_rays=0), False, 0, 1, REFILL),
                      (dict(refill=t, persistent=1, min_rays=0), False, mid, 0, REFILL),
                      (dict(refill=(0, 0), persistent=1, min_rays=0), False, mid, 1, "k_trace_persist<0>"),
                      (dict(refill=t, persistent=1, min_rays=0), False, n, 0, REFILL)]
        for options, both, coherent_from, aos, kernel in cases:
            rig.configure(**options)
            for rep in range(2):
                what = (name, set_name, options, both, coherent_from, aos, rep)
                rig.r.clear()
                before = rig.r.counters()["shadow_rays"]
                rig.check_primary(first, lambda: rig.streams(True, coherent_from, both, None, aos), kernel, aos=bool(aos), what=what)
                if both:
                    film = rig.r.film().reshape(-1, 3)
                    assert np.array_equal(film[:rig.pixels], rig.film_of(rays, ids, colours, n_s)), what
                    assert rig.r.counters()["shadow_rays"] - before == int((ids >= 0).sum()), what


@pytest.mark.parametrize("name", CLASSES)
def test_streams_that_are_no_slabs_fall_back_to_whole_chunks(rig_for, name):
    """Two hit arrays (or two colour arrays) of a stream moved elsewhere: the lane refill, which addresses a stream as one slab, is not
    used -- k_trace_persist takes the launch and writes through the struct's pointers; 20-byte records on such a stream are refused and
    nothing is enqueued."""
    import torch
    rig = rig_for(name)
    set_name = "specials"
    rays = rig.h.ray_sets[set_name]
    n = len(rays) - 37
    first = np.ascontiguousarray(rays[:n])
    ids, colours = X.dead_ray_ids(len(rays)), colours_for(len(rays))
    rig.load_primary(first); rig.load_shadow(rays, ids, colours)
    elsewhere = [torch.zeros(rig.cap, dtype=torch.int32, device="cuda") for _ in range(4)]
    old = (rig.p.t, rig.p.u, rig.s.color_r, rig.s.color_b)
    rig.configure(refill=(40, 40), persistent=1, min_rays=0)
    rig.check_primary(first, lambda: rig.streams(True, 0, True), REFILL, what="slabs")
    try:
        rig.p.t, rig.p.u = elsewhere[0].data_ptr(), elsewhere[1].data_ptr()
        moved = {"t": rig.p.t, "u": rig.p.u}
        for rep in range(2):
            rig.check_primary(first, lambda: rig.streams(True, 0, True), "k_trace_persist<2>", moved=moved, what=("moved", rep))
            rig.check_primary(first, lambda: rig.streams(True, 0, False), "k_trace_persist<0>", moved=moved, what=("moved", rep))
        # refused: the record memory keeps its poison and the kernel name is the last launch's
        rig.check_primary(first, lambda: rig.streams(True, 0, False), "k_trace_persist<0>", moved=moved, what="before the refusal")
        rig.R.write_stream_array(rig.p.geom_id, np.full(5 * rig.cap, POISON, "<u4"))
        before = rig.r.counters()
        rig.streams(True, 0, True, flags=1, expect_status=-4)
        assert (rig.R.read_stream_array(rig.p.geom_id, 5 * rig.cap, "<u4") == POISON).all() and rig.r.counters() == before
        rig.p.t, rig.p.u = old[0], old[1]
        rig.s.color_r, rig.s.color_b = elsewhere[2].data_ptr(), elsewhere[3].data_ptr()
        rig.R.write_stream_array(rig.s.color_r, colours[:, 0]); rig.R.write_stream_array(rig.s.color_b, colours[:, 2])
        rig.check_shadow(rays, ids, colours, rig.secondary_entry, "k_trace_persist<1>", what="colours moved")
        rig.check_shadow(rays, ids, colours, lambda: rig.streams(False, 0, True), "k_trace_persist<1>", what="colours moved")
    finally:
        rig.p.t, rig.p.u, rig.s.color_r, rig.s.color_b = old
    rig.check_shadow(rays, ids, colours, rig.secondary_entry, REFILL, what="slab again")


SIZE_ROUTES = {"one-chunk": (dict(lds_image=1), None), "persist": (dict(refill=(0, 0)), "k_trace_persist<2>"),
               "refill-40": (dict(refill=(40, 40)), REFILL), "refill-1": (dict(refill=(1, 1)), REFILL)}


@pytest.mark.parametrize("route", SIZE_ROUTES)
def test_list_sizes_around_a_wave_and_a_ticket_group(rig_for, route):
    """Both lists at 1, 63, 64, 65, 2047, 2048 and 2049 rays (a wave is 64 rays, a ticket group of the persistent kernels 32 chunks), on
    the soup: the last ray is traced, nothing behind it is written."""
    rig = rig_for("soup")
    options, kernel = SIZE_ROUTES[route]
    rig.configure(**options)
    segments = rig.h.ray_sets["segments"]
    colours = colours_for(len(segments))
    for n in X.EDGE_SIZES:
        rays = X.take(segments, n)
        ids = np.arange(n, dtype="<i4")
        rig.load_primary(rays); rig.load_shadow(rays, ids, colours[:n])
        for rep in range(2):
            what = (route, n, rep)
            if kernel is None:
                rig.check_primary(rays, rig.primary_entry, "k_trace_primary<2,31>", what=what)
                rig.check_shadow(rays, ids, colours[:n], rig.secondary_entry, "k_trace_secondary<2,31>", what=what)
            else:
                rig.r.clear()
                rig.check_primary(rays, lambda: rig.streams(True, (n // 2) | 1 if n > 1 else 0, True), kernel, what=what)
                assert np.array_equal(rig.r.film().reshape(-1, 3)[:rig.pixels], rig.film_of(rays, ids, colours[:n], n)), what


def test_second_ticket_row_on_the_cornell_box(rig_for):
    """131 072 + 65 rays in both lists: a stripe's tickets beyond its first 2048 lead into the second row of index_of (k_trace_refill) and
    of the 32-chunk groups (k_trace_persist)."""
    n = X.SECOND_ROW_SIZE
    rig = rig_for("cornell", capacity=n, pixels=n)
    rays = X.take(rig.h.ray_sets["random"], n)
    ids, colours = X.dead_ray_ids(n), colours_for(n)
    rig.load_primary(rays); rig.load_shadow(rays, ids, colours)
    for options, kernel in ((dict(refill=(40, 40)), REFILL), (dict(refill=(0, 0)), "k_trace_persist<2>")):
        rig.configure(**options)
        rig.r.clear()
        rig.check_primary(rays, lambda: rig.streams(True, n // 2 | 1, True), kernel, what=kernel)
        assert np.array_equal(rig.r.film().reshape(-1, 3)[:n], rig.film_of(rays, ids, colours, n)), kernel


DEAD_ROUTES = {"one-chunk-image": (dict(lds_image=1), False, "k_trace_secondary<2,31>"),
               "one-chunk-plain": (dict(lds_image=0), False, "k_trace_secondary<1,0>"),
               "persist<1>": (dict(persistent=1, min_rays=0), False, "k_trace_persist<1>"),
               "refill-shadow-only": (dict(persistent=1, min_rays=0, refill=(32, 32)), False, REFILL),
               "persist<2>": (dict(refill=(0, 0)), True, "k_trace_persist<2>"),
               "refill-joint": (dict(refill=(40, 40)), True, REFILL)}


@pytest.mark.parametrize("route", DEAD_ROUTES)
def test_dead_shadow_rays_and_a_size_on_the_device(rig_for, oracle, route):
    """Dead shadow rays (id -1) in lanes 0 and 63, in whole waves, in every second lane and in the last, partial wave, and the list's size
    read from device memory: all of it, one ray less, the middle of a wave, nothing.  The rays behind the size are alive and finite -- the
    first of them unoccluded -- and add nothing to the film or the counter."""
    import torch
    rig = rig_for("soup")
    options, with_primary, kernel = DEAD_ROUTES[route]
    rig.configure(**options)
    n = X.dead_case_size(oracle)
    rays = X.take(rig.h.ray_sets["segments"], n)
    ids, colours = X.dead_ray_ids(n), colours_for(n)
    first = np.ascontiguousarray(rays[:n - 100])
    rig.load_primary(first); rig.load_shadow(rays, ids, colours)
    for size in X.device_sizes(n) + (n,):
        size_dev = torch.tensor([size], dtype=torch.int32, device="cuda")
        what = (route, size)
        if with_primary:
            rig.check_shadow(rays, ids, colours, lambda: rig.streams(True, 0, True, size_dev), kernel, size=size, what=what)
            region = rig.R.read_stream_array(rig.p.prim_id, len(first), "<i4")
            assert np.array_equal(region, rig.records(first)[1]), what
        else:
            rig.check_shadow(rays, ids, colours, lambda: rig.streams(False, 0, True, size_dev), kernel, size=size, what=what)
    rig.check_shadow(rays, ids, colours, lambda: rig.streams(with_primary, 0, True, None), kernel, what=(route, "host size"))


@pytest.mark.parametrize("route", ["one-chunk-image", "persist<1>", "refill-joint"])
def test_rays_that_share_pixels(rig_for, oracle, route):
    """film_add_wave: 64 lanes on one pixel, two pixels to a wave, six pixels with repeats (more than the kFilmRounds = 4 it sums in the
    wave: the rest fall back to their own atomics), a pixel shared by several waves, and all of that with dead and occluded lanes between.
    Against the fp64 sum of the fp32 contributions, within the bound of an fp32 sum of k terms in any order: gamma_(k-1) x sum |c_i|
    (stream_trace_fixtures.film_sum_bound) -- no other tolerance."""
    rig = rig_for("soup")
    options, with_primary, kernel = DEAD_ROUTES[route]
    rig.configure(**options)
    n = 64 * 24 + 40
    rays = X.take(rig.h.ray_sets["segments"], n)
    i = np.arange(n)
    w, lane = i // 64, i % 64
    ids = np.select([w % 4 == 0, w % 4 == 1, w % 4 == 2], [0 * i, 1 + lane % 2, 3 + (lane * 7) % 6], 9 + (lane // 16)).astype("<i4")
    ids[(w >= 12) & (lane % 5 == 0)] = -1
    colours = colours_for(n, 3)
    num_pixels = 13
    rig.load_primary(rays); rig.load_shadow(rays, ids, colours)
    want = X.expected_film(oracle, rig.h.scene, rays, ids, colours, 1.0, n, rig.pixels)
    bound = X.film_sum_bound(oracle, rig.h.scene, rays, ids, colours, 1.0, n, rig.pixels)
    assert (want[:num_pixels] > 0).all() and not want[num_pixels:].any() and (bound[:num_pixels] > 0).all()
    for rep in range(2):
        rig.r.clear()
        before = rig.r.counters()["shadow_rays"]
        rig.streams(with_primary, 0, True)
        assert rig.kernel() == kernel
        film = rig.r.film().reshape(-1, 3).astype(np.float64)
        error = np.abs(film[:rig.pixels] - want)
        print(route, rep, "largest error / bound", float((error[:num_pixels] / bound[:num_pixels]).max()))
        assert (error <= bound).all(), (route, rep, error[:num_pixels], bound[:num_pixels])
        assert rig.r.counters()["shadow_rays"] - before == int((ids >= 0).sum())


def test_bad_arguments_enqueue_nothing(rig_for):
    rig = rig_for("cornell")
    rays = rig.h.ray_sets["edge"]
    rig.load_primary(rays); rig.load_shadow(rays, np.arange(len(rays)), colours_for(len(rays)))
    rig.check_primary(rays, rig.primary_entry, "k_trace_primary<2,31>")
    rig.R.write_stream_array(rig.p.geom_id, np.full(5 * rig.cap, POISON, "<u4"))
    rig.r.clear()
    before = rig.r.counters()
    rig.streams(False, 0, False, expect_status=-1)
    rig.streams(True, 0, True, flags=2, expect_status=-2)
    rig.streams(True, len(rays) + 1, True, expect_status=-3)
    rig.streams(False, 0, True, flags=1, expect_status=-4)
    assert rig.kernel() == "k_trace_primary<2,31>" and rig.r.counters() == before and not rig.r.film().any()
    assert (rig.R.read_stream_array(rig.p.geom_id, 5 * rig.cap, "<u4") == POISON).all()
    rig.check_primary(rays, lambda: rig.streams(True, len(rays), False), "k_trace_primary<2,31>")      # coherent_from == size is fine


def test_defaults_put_the_persistent_threshold_back(rig_for, R):
    rig = rig_for("cornell")
    rays = X.take(rig.h.ray_sets["random"], 1000)
    rig.load_primary(rays)
    assert rig.r.persist_min_rays() == 8192 * 64
    rig.configure(persistent=1, min_rays=0)
    assert rig.r.persist_min_rays() == 0
    rig.check_primary(rays, rig.primary_entry, "k_trace_persist<0>")
    assert rig.r.persist_min_rays(-1) == 8192 * 64 and rig.r.persist_min_rays(77) == 77
    R.lib().rodent_hip_render_defaults(0)
    assert rig.r.persist_min_rays() == 8192 * 64
    R.lib().rodent_hip_render_trace_persistent(0, 1)
    rig.check_primary(rays, rig.primary_entry, "k_trace_primary<2,31>")
    rig.close()
    again = R.Renderer(rig.h.scene, 64, 64, 1, 4, trace_persistent=1, persist_min_rays=500)
    assert again.persist_min_rays() == 500
    rig.r = again                                                # closed by the fixture


# ---- the switches a process reads once ------------------------------------------------------------------------------------------------
def child():
    """The joint lane-refill route on the soup with the specials and the segments, in a process whose environment chose the kernel; prints
    the kernel's name."""
    from oracle import binding
    from rodent_amd import render
    rig = Rig(render, binding, X.hierarchy("soup"))
    names = set()
    for set_name in ("specials", "segments"):
        rays = rig.h.ray_sets[set_name]
        n = len(rays) - 37
        first = np.ascontiguousarray(rays[:n])
        ids, colours = X.dead_ray_ids(len(rays)), colours_for(len(rays))
        rig.load_primary(first); rig.load_shadow(rays, ids, colours)
        for t in ((40, 40), (1, 1)):
            rig.configure(refill=t)
            for coherent_from, aos in ((0, 0), ((n // 2) | 1, 1), (n, 0)):
                rig.r.clear()
                rig.streams(True, coherent_from, True, None, aos)
                names.add(rig.kernel())
                rig.check_primary(first, lambda: rig.streams(True, coherent_from, True, None, aos), rig.kernel(), aos=bool(aos),
                                  what=(set_name, t, coherent_from, aos))
                film = rig.r.film().reshape(-1, 3)
                # two launches: every lit pixel twice (x + x is exact)
                assert np.array_equal(film[:rig.pixels], 2 * rig.film_of(rays, ids, colours, len(rays))), (set_name, t, coherent_from)
    rig.close()
    print("KERNEL", ",".join(sorted(names)) if len(names) == 1 else sorted(names))


@pytest.mark.parametrize("variable,value,kernel", [("RODENT_HIP_SHADOW_ORDER", "0", "k_trace_refill<0,true>"),
                                                   ("RODENT_HIP_SHADOW_ORDER", "2", "k_trace_refill<2,true>"),
                                                   ("RODENT_HIP_LAZY_MISS", "0", "k_trace_refill<1,false>")])
def test_switches_read_once_per_process(native_build, variable, value, kernel):
    """The shadow order and the form of the miss record are read once per process: one fresh child per setting runs the joint lane-refill
    route on the soup (specials: the miss record's tmax bit for bit whichever form stores it; segments), and names the kernel that ran --
    every shadow order has the lazy form."""
    env = {k: v for k, v in os.environ.items() if k not in ("RODENT_HIP_SHADOW_ORDER", "RODENT_HIP_LAZY_MISS")}
    env[variable] = value
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"KERNEL {kernel}\n" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    child()
