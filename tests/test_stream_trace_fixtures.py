"""What tests/test_gpu_render_trace.py relies on, checked on the CPU with the oracle alone: a comparison of hit records proves little on a
ray set that only hits or only misses, a spill-block edge nobody's stack reaches tests nothing, and a signalling NaN that never ends up in
a miss record cannot show whether the record keeps its bits."""
import numpy as np
import pytest

import stream_trace_fixtures as X


@pytest.fixture(scope="module")
def outcomes(oracle):
    """{(hierarchy, ray set): (closest-hit mask, any-hit mask, deepest stacks closest hit, ... any hit)}"""
    out = {}
    for name in X.HIERARCHIES:
        h = X.hierarchy(name, oracle)
        for set_name, rays in h.ray_sets.items():
            closest, _ = oracle.traverse(2, h.nodes, h.tris, rays)
            occluded, _ = oracle.traverse(2, h.nodes, h.tris, rays, any_hit=True)
            out[name, set_name] = (closest["tri_id"] >= 0, occluded["tri_id"] >= 0, oracle.ray_depths(h.nodes, h.tris, rays),
                                   oracle.ray_depths(h.nodes, h.tris, rays, any_hit=True))
    return out


def test_every_pair_of_hierarchy_and_ray_set_hits_and_misses(outcomes):
    assert {h for h, _ in outcomes} == set(X.HIERARCHIES)
    for key, (hit, occluded, _, _) in outcomes.items():
        for mask in (hit, occluded):
            assert 0.2 <= mask.mean() <= 0.8, (key, mask.mean())


def test_ray_sets_hold_a_few_thousand_rays_of_every_kind(oracle):
    for name in X.HIERARCHIES:
        h = X.hierarchy(name, oracle)
        assert set(h.ray_sets) == {"cornell": {"edge", "random", "specials", "axis"}, "soup": {"segments", "specials", "axis"},
                                   "padded": {"segments", "specials", "axis"}}.get(name, {"chain", "chain_jitter"})
        for set_name, rays in h.ray_sets.items():
            assert len(rays) <= 4096 and (set_name == "edge" or len(rays) >= 1000), (name, set_name, len(rays))
    assert X.hierarchy("soup").ray_sets["segments"].tobytes() == X.hierarchy("padded", oracle).ray_sets["segments"].tobytes()
    axis = X.hierarchy("soup").ray_sets["axis"]
    zeros = (axis["dir"] == 0).sum(1)
    assert set(zeros) == {1, 2}
    # zeros of either sign
    assert np.signbit(axis["dir"][axis["dir"] == 0]).any() and not np.signbit(axis["dir"][axis["dir"] == 0]).all()
    lo, hi = X.root_box(X.hierarchy("soup").nodes)
    lo, hi = lo.astype("<f4"), hi.astype("<f4")
    inside = ((axis["org"] > lo) & (axis["org"] < hi)).all(1)
    on_face = (((axis["org"] == lo) | (axis["org"] == hi)).any(1)) & ((axis["org"] >= lo) & (axis["org"] <= hi)).all(1)
    outside = ((axis["org"] < lo) | (axis["org"] > hi)).any(1)
    assert min(inside.sum(), on_face.sum(), outside.sum()) >= 200
    jitter = X.hierarchy("chain40").ray_sets["chain_jitter"]["dir"]
    assert len(np.unique(jitter, axis=0)) == len(jitter) and len(np.unique(X.hierarchy("chain40").ray_sets["chain"]["dir"], axis=0)) == 1


def test_hierarchy_classes(oracle):
    cornell, soup, padded = (X.hierarchy(n, oracle) for n in ("cornell", "soup", "padded"))
    assert len(cornell.nodes) <= 31                              # whole tree inside both LDS images
    assert len(soup.nodes) > 255 and len(soup.tris) == X.SOUP_TRIANGLES      # image links lead into memory
    assert set(np.unique(soup.tris["geom_id"])) == set(range(X.SOUP_GEOMETRIES)) and soup.num_materials == X.SOUP_GEOMETRIES
    c = X.triangle_corners(soup.tris)
    points = (c[:, 0] == c[:, 1]).all(1) & (c[:, 0] == c[:, 2]).all(1)
    lines = ~points & ((c[:, 1] == c[:, 2]).all(1))
    assert points.sum() > 100 and lines.sum() > 100
    # rays whose closest hit lies on three triangles at once: their record tells the order of the visits
    copies = X.copied_triangles()
    for set_name, rays in soup.ray_sets.items():
        closest = oracle.traverse(2, soup.nodes, soup.tris, rays)[0]
        assert np.isin(closest["tri_id"], copies).sum() >= 50, set_name
        assert len(set(closest["tri_id"][np.isin(closest["tri_id"], copies)] % 13)) == 3 or set_name == "axis", set_name
    # a zero direction component must not turn the slab distances into NaN for every box (see soup_mesh)
    assert np.abs(np.concatenate(X.root_box(soup.nodes))).max() < 1.0
    assert len(padded.nodes) == len(soup.nodes) + X.padding_levels(oracle) + 1 and padded.tris is soup.tris
    # whatever order a kernel visits the children in (the shadow rays' differs from the oracle's), no stack outgrows the 63 entries every
    # stack of the stream kernels holds: no test raises the overflow flag
    for name in X.HIERARCHIES:
        assert X.tree_depth(X.hierarchy(name, oracle).nodes) <= 63, name


def test_stack_depths_meet_every_spill_block_edge(outcomes, oracle):
    """Closest hit: the padded soup's deepest stacks span 14 ... 30 entries with every edge present; any hit, in the oracle's order (the
    nearer child first, RODENT_HIP_SHADOW_ORDER=0): the first two edges at least.  (In the kernels' default order a shadow ray takes child
    0 first and is out of a wrapper at once: the chains are what takes shadow rays over the edges in every order.)  A chain's +z rays
    hold exactly its depth, closest hit and any hit, the reference's capacity (63 entries) at most."""
    closest = np.concatenate([outcomes["padded", s][2] for s in X.hierarchy("padded", oracle).ray_sets])
    shadow = np.concatenate([outcomes["padded", s][3] for s in X.hierarchy("padded", oracle).ray_sets])
    entered = closest[closest > 0]
    assert entered.min() <= X.PADDED_DEPTH_SPAN[0] and entered.max() == X.PADDED_DEPTH_SPAN[1]
    assert set(X.SPILL_EDGE_DEPTHS) <= set(entered.tolist())
    assert {15, 16, 22, 23} <= set(shadow.tolist())
    unpadded = max(outcomes["soup", s][2].max() for s in X.hierarchy("soup").ray_sets)
    assert X.padding_levels(oracle) == X.PADDED_DEPTH_SPAN[1] - unpadded > 0
    for d in X.CHAIN_DEPTHS:
        for s in ("chain", "chain_jitter"):
            hit, _, depth, any_depth = outcomes[f"chain{d}", s]
            assert depth.max() == d <= 63 and (depth[hit] == d).all() and any_depth.max() == d
            assert not hit[::3].any() and hit[1::3].all() and hit[2::3].all()               # every third ray misses


def test_special_values_reach_miss_records_and_hits(outcomes, oracle):
    """Every pair of the 12 x 12 table lies over rays of both kinds; missed rays carry a signalling NaN and a denormal as tmax (what the
    miss record must keep bit for bit), and hits exist under every tmin / tmax that can accept one."""
    m = len(X.SPECIALS)
    for name in ("cornell", "soup", "padded"):
        rays = X.hierarchy(name, oracle).ray_sets["specials"]
        hit = outcomes[name, "specials"][0]
        tmin, tmax = rays["tmin"].view("<u4"), rays["tmax"].view("<u4")
        pairs = {(a, b) for a, b in zip(tmin.tolist(), tmax.tolist())}
        assert len(pairs) == m * m
        for bits in (X.SNAN_BITS, X.DENORMAL_BITS, 0xFFC12345, 0x7FC00000):
            assert (~hit & (tmax == bits)).sum() >= 20, (name, hex(bits))
        accepted = {(a, b) for a, b in zip(tmin[hit].tolist(), tmax[hit].tolist())}
        want = {(int(X.SPECIALS.view("<u4")[a]), int(X.SPECIALS.view("<u4")[b])) for a in X.ACCEPTING_TMIN for b in X.ACCEPTING_TMAX}
        assert want <= accepted, (name, want - accepted)
        # with a plain interval, three in four of these rays hit and one in four misses
        plain = rays.copy(); plain["tmin"] = 0.0; plain["tmax"] = 1.0
        plain_hit = oracle.traverse(2, X.hierarchy(name, oracle).nodes, X.hierarchy(name, oracle).tris, plain)[0]["tri_id"] >= 0
        k = np.arange(len(rays))
        for residue in range(m * m):
            assert plain_hit[k % (m * m) == residue].any() and not plain_hit[k % (m * m) == residue].all()


def test_expected_records_and_film(oracle):
    h = X.hierarchy("soup")
    rays = h.ray_sets["specials"]
    geom, prim, t, u, v = X.expected_records(oracle, h.scene, rays)
    hit = prim >= 0
    assert (geom[~hit] == h.num_materials).all() and (u[~hit] == 0).all() and (v[~hit] == 0).all()
    assert t[~hit].tobytes() == rays["tmax"][~hit].tobytes()
    of_prim = X.geometry_of_primitive(h.tris)
    assert (of_prim >= 0).all() and (geom[hit] == of_prim[prim[hit]]).all() and len(set(geom[hit].tolist())) == X.SOUP_GEOMETRIES
    # the film counts rays in front of n that are alive and unoccluded, once each
    seg = h.ray_sets["segments"]
    n = len(seg)
    ids = X.dead_ray_ids(n)
    colours = np.random.default_rng(0).uniform(0.1, 1.0, (n, 3)).astype("<f4")
    occluded = oracle.traverse(2, h.nodes, h.tris, seg, any_hit=True)[0]["tri_id"] >= 0
    for size in X.device_sizes(n):
        film = X.expected_film(oracle, h.scene, seg, ids, colours, 1.0, size, n)
        lit = (ids >= 0) & ~occluded & (np.arange(n) < size)
        assert np.array_equal(film.astype("<f4"), np.where(lit[:, None], colours, np.float32(0)))
        assert (X.film_sum_bound(oracle, h.scene, seg, ids, colours, 1.0, size, n) == 0).all()       # one contribution: exact
    shared = (np.arange(n) % 5).astype("<i4")
    bound = X.film_sum_bound(oracle, h.scene, seg, shared, colours, 0.25, n, 5)
    film = X.expected_film(oracle, h.scene, seg, shared, colours, 0.25, n, 5)
    k = np.bincount(shared[~occluded], minlength=5)[:, None]
    assert (bound > 0).all() and np.allclose(bound, (k - 1) * 2.0 ** -24 * film, rtol=1e-4)      # positive colours: sum |c| = the sum


def test_sizes_and_dead_ray_patterns_are_constructible(oracle, outcomes):
    soup = X.hierarchy("soup")
    assert len(soup.ray_sets["segments"]) >= max(X.EDGE_SIZES) + 1000
    hit, occluded = outcomes["soup", "segments"][:2]
    for n in X.EDGE_SIZES:                                       # the last ray of every size, and the one behind it, are not all alike
        assert len(X.take(soup.ray_sets["segments"], n)) == n
    assert len({bool(hit[n - 1]) for n in X.EDGE_SIZES}) == 2 and len({bool(occluded[n - 1]) for n in X.EDGE_SIZES}) == 2
    big = X.take(X.hierarchy("cornell").ray_sets["random"], X.SECOND_ROW_SIZE)
    assert len(big) == X.SECOND_ROW_SIZE == 64 * 2048 + 65
    assert big[-1].tobytes() == X.hierarchy("cornell").ray_sets["random"][(X.SECOND_ROW_SIZE - 1) % 4096].tobytes()
    n = X.dead_case_size(oracle)
    assert n > 2049 and n % 64 > 1
    ids = X.dead_ray_ids(n)
    waves = ids[: n // 64 * 64].reshape(-1, 64)
    dead = waves < 0
    assert (dead[:, [0, 63]].all(1) & (dead.sum(1) == 2)).sum() >= 4                          # lanes 0 and 63
    assert dead.all(1).sum() >= 4                                                            # whole waves
    assert ((dead[:, 1::2].all(1)) & (~dead[:, 0::2]).all(1)).sum() >= 4                      # every second lane
    tail = ids[n // 64 * 64:]
    assert 0 < len(tail) < 64 and (tail < 0).any() and (tail >= 0).any()                     # the last, partial wave
    assert (ids[ids >= 0] == np.flatnonzero(ids >= 0)).all()                                 # one pixel per live ray
    sizes = X.device_sizes(n)
    assert sizes[0] == n and sizes[1] == n - 1 and sizes[2] % 64 not in (0, 63) and 0 < sizes[2] < n - 64 and sizes[3] == 0
    # the first ray behind every size is alive and unoccluded: it would show in the film if the kernel traced it
    rays = X.take(soup.ray_sets["segments"], n)
    lit = (ids >= 0) & ~(oracle.traverse(2, soup.nodes, soup.tris, rays, any_hit=True)[0]["tri_id"] >= 0)
    for size in sizes[1:3]:
        assert lit[size], size
    assert lit[:64].sum() > 10                                   # size 0: the first wave alone would show
