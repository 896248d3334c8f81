"""Hierarchies, ray sets and expected results for the tests of the renderer's stream traversal kernels (rodent_amd/csrc/render_trace.h).

Plain numpy: tests/test_stream_trace_fixtures.py checks on the CPU, with the oracle alone, every condition the GPU tests of
tests/test_gpu_render_trace.py rely on (hit and miss shares, node counts, stack depths, the special values that reach a miss record).

Three classes of hierarchy:
* "cornell": the committed Cornell box, about 20 nodes -- the whole tree sits inside both LDS images (31 and 255 records);
* "soup": the device builder's model (lbvh_model.build, max_leaf 2) of a seeded 3000-triangle soup with point and line triangles and four
  geometry ids -- more than 255 nodes, so image links lead into memory;
* "padded": the soup under pad_bvh2_depth(levels), `levels` derived from the oracle's stack depths so that the deepest stacks of the
  soup's rays span 14 ... 30 entries and meet every edge of the persistent kernels' spill blocks (15 + 7 k); and "chain16" ... "chain63":
  chain_bvh2(d), whose +z rays hold exactly d entries (63 = the capacity of every stack of the stream kernels: 14 entries in the 15-row
  window + 7 blocks of 7 behind it, stack_spill; 64 slots of k_trace_deep's stack, of which a ray on the chain writes slots 0 ... 63).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import lbvh_model
from conftest import GOLDEN, chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F
from rodent_amd import scene as S

# tmin / tmax of test_gpu_parity.test_special_tmin_tmax_values: 0, -0, denormal, +-inf, quiet NaN, signalling NaN, negative NaN with a
# payload, 5, -1, 0.01, FLT_MAX
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345,
                     0x40A00000, 0xBF800000, 0x3C23D70A, 0x7F7FFFFF], dtype="<u4").view("<f4")
SNAN_BITS, DENORMAL_BITS = 0x7FA00001, 0x00000001
CHAIN_DEPTHS = (16, 23, 40, 63)
# the first entry the persistent kernels move out of their window, and both sides of every block edge below the padded soup's deepest stack
SPILL_EDGE_DEPTHS = (15, 16, 22, 23, 29, 30)
PADDED_DEPTH_SPAN = (14, 30)
HIERARCHIES = ("cornell", "soup", "padded") + tuple(f"chain{d}" for d in CHAIN_DEPTHS)
SOUP_TRIANGLES, SOUP_GEOMETRIES, SOUP_SEED = 3000, 4, 20


def scene_of(nodes, tris, num_materials):
    """The hand-made scene of a hierarchy alone: one light, zero vertex tables, `num_materials` diffuse materials.  Good for traversal
    (hit records, shadow rays into the film); nothing here can be shaded."""
    ntri = len(tris)
    mat = np.zeros(num_materials, S.MATERIAL); mat["kd"] = 0.5; mat["type"] = 1
    light = np.zeros(1, S.LIGHT); light["inv_area"] = 1.0
    return SimpleNamespace(vertices=np.zeros((3 * ntri, 4), "<f4"), normals=np.zeros((3 * ntri, 4), "<f4"),
                           face_normals=np.zeros((ntri, 4), "<f4"), indices=np.zeros((ntri, 4), "<i4"), nodes=nodes, tris=tris,
                           materials=mat, lights=light, light_ids=np.zeros(ntri, "<i4"), texcoords=np.zeros((0, 4), "<f4"),
                           textures=np.zeros(0, S.TEXTURE), texels=np.zeros(0, "<u4"), num_tris=ntri)


def root_box(nodes):
    """(lo, hi) of the root's two child boxes."""
    b = nodes[0]["bounds"].astype(np.float64)
    lo = np.minimum(b[0:6:2], b[6:12:2]); hi = np.maximum(b[1:6:2], b[7:12:2])
    return lo, hi


def soup_mesh(n=SOUP_TRIANGLES, seed=SOUP_SEED):
    """n triangles over 3n vertices: half of them spread over a box of side 0.8 about the origin, half in clusters that shrink towards one
    corner (the Morton order then has a long spine: stacks a dozen and a half entries deep), with degenerate ones (a point, a line) mixed
    in as test_gpu_build.soup does, triangles that lie three to a place, and geometry ids 0 ... 3 in indices[:, 3]."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10, 10, (n, 1, 3))
    scale = np.full((n, 1, 1), 0.9)
    k = np.arange(n // 2, n)
    level = rng.integers(0, 14, len(k))
    shrink = 0.5 ** level
    centre[k, 0] = -10 + 20 * shrink[:, None] * rng.uniform(0.5, 1.0, (len(k), 3))
    scale[k, 0, 0] = 3.0 * shrink
    # inside the unit box: a ray with a zero direction component has the reciprocal +-FLT_MAX there (safe_rcp), and o x FLT_MAX is finite
    # only for |o| < 1 -- further out the slab distances of that axis are NaN and the ray misses nearly every box, in the reference too
    corners = 0.04 * (centre + scale * rng.normal(0, 1, (n, 3, 3)))
    v = np.zeros((3 * n, 4), np.float32)
    v[:, :3] = corners.reshape(-1, 3).astype(np.float32)
    pts = np.arange(0, n, 7)                                     # degenerate: all three corners in one point
    v[3 * pts + 1], v[3 * pts + 2] = v[3 * pts], v[3 * pts]
    lines = np.arange(3, n, 11)                                  # degenerate: a line
    v[3 * lines + 2] = v[3 * lines + 1]
    # three triangles on the same corners, each with its own id: with two triangles to a leaf they cannot share one, and a ray through them
    # is accepted three times at the same t (t <= tmax) -- which id its record ends with depends on the order of the visits
    first = np.arange(2, n - 2, 13)
    for copy in (1, 2):
        for corner in range(3):
            v[3 * (first + copy) + corner] = v[3 * first + corner]
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    ix[:, 3] = rng.integers(0, SOUP_GEOMETRIES, n)
    return v, ix


def copied_triangles(n=SOUP_TRIANGLES):
    """Ids of the soup's triangles that lie three to a place (soup_mesh)."""
    first = np.arange(2, n - 2, 13)
    return np.sort(np.concatenate([first, first + 1, first + 2]))


def tree_depth(nodes):
    """Inner nodes on the longest path from the root: no visit order can hold more stack entries than that."""
    depth = np.zeros(len(nodes) + 1, np.int64)
    order, todo = [], [1]
    while todo:
        k = todo.pop()
        order.append(k)
        todo += [int(c) for c in nodes[k - 1]["child"] if c > 0]
    for k in reversed(order):
        depth[k] = 1 + max([depth[int(c)] for c in nodes[k - 1]["child"] if c > 0], default=0)
    return int(depth[1])


def triangle_corners(tris):
    """(n, 3, 3) float64 corners of Tri1 records (e1 = v0 - v1, e2 = v2 - v0)."""
    v0 = tris["v0"].astype(np.float64)
    return np.stack([v0, v0 - tris["e1"], v0 + tris["e2"]], 1)


# ---- ray sets ------------------------------------------------------------------------------------------------------------------------
def segment_rays(nodes, tris, n, seed):
    """Segments (tmin 0, tmax 1) through the hierarchy's box: every second one is aimed at a point of a triangle and ends behind it or,
    one time in three, in front of it; the others join two random points of the box grown by a quarter."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(nodes)
    grow = 0.25 * (hi - lo)
    org = rng.uniform(lo - grow, hi + grow, (n, 3))
    end = rng.uniform(lo - grow, hi + grow, (n, 3))
    target = _aim_points(nodes, tris, rng, n, (1.0, 1.0, 1.0))
    reach = np.where(rng.random(n) < 1 / 3, rng.uniform(0.2, 0.95, n), rng.uniform(1.05, 2.0, n))
    aimed = np.arange(n) % 2 == 0
    d = np.where(aimed[:, None], (target - org) * reach[:, None], end - org)
    # every eighth one starts near the box's low corner, as near again as often as not, and runs out of the box: where triangles crowd
    # into that corner ever smaller (soup_mesh) it leaves one entry on its stack for every box it starts in -- the deepest stacks
    spine = np.flatnonzero(np.arange(n) % 8 == 1)
    org[spine] = lo + (hi - lo) * 0.5 ** rng.integers(1, 15, (len(spine), 1)) * rng.uniform(0.3, 1.0, (len(spine), 3))
    d[spine] = (lo + (hi - lo) * rng.uniform(0.3, 1.2, (len(spine), 3)) - org[spine])
    return F.make_rays(org.astype("<f4"), d.astype("<f4"), 0.0, 1.0)


# the values the triangle test's comparisons t >= tmin, t <= tmax can accept for a t in (0.01, 5): indices into SPECIALS
ACCEPTING_TMIN, ACCEPTING_TMAX = (0, 1, 2, 4, 9, 10), (3, 8, 11)


def _aim_points(nodes, tris, rng, n, weights):
    """n points on triangles that have an area (degenerate ones cannot be hit)."""
    lo, hi = root_box(nodes)
    c = triangle_corners(tris)
    area = np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)
    c = c[np.isfinite(area) & (area > 1e-6 * float((hi - lo).max()) ** 2)]
    w = rng.dirichlet(weights, n)
    return (c[rng.integers(0, len(c), n)] * w[:, :, None]).sum(1)


def special_rays(nodes, tris, seed, repeats=8):
    """The 12 x 12 tmin x tmax table of SPECIALS laid `repeats` times over rays of which three in four end behind a point of a triangle
    they are aimed at (t <= 1 there) and one in four misses everything: ray k has tmin SPECIALS[k % 12], tmax SPECIALS[(k // 12) % 12],
    and the kind of ray changes with k // 144 and k, so every pair of values meets both kinds.  Only 18 of the 144 pairs leave a hit
    possible (ACCEPTING_*), so behind the table come as many rays again whose pairs are those 18 in turn: both outcomes are well
    represented."""
    rng = np.random.default_rng(seed)
    m = len(SPECIALS)
    table = m * m * repeats
    n = 2 * table
    lo, hi = root_box(nodes)
    size = hi - lo
    target = _aim_points(nodes, tris, rng, n, (2.0, 2.0, 2.0))
    org = rng.uniform(lo + 0.05 * size, hi - 0.05 * size, (n, 3))
    d = (target - org) * rng.uniform(1.1, 1.6, (n, 1))
    k = np.arange(n)
    away = (k // (m * m) + k) % 4 == 3                         # these start outside the box and point away from it
    org[away] = hi + size * rng.uniform(0.5, 1.5, (int(away.sum()), 3))
    d[away] = np.abs(d[away]) + 0.01 * size
    rays = F.make_rays(org.astype("<f4"), d.astype("<f4"))
    j = k - table                                              # behind the table
    tmin_index = np.where(k < table, k % m, np.array(ACCEPTING_TMIN)[j % len(ACCEPTING_TMIN)])
    tmax_index = np.where(k < table, (k // m) % m, np.array(ACCEPTING_TMAX)[(j // len(ACCEPTING_TMIN)) % len(ACCEPTING_TMAX)])
    rays["tmin"] = SPECIALS[tmin_index]
    rays["tmax"] = SPECIALS[tmax_index]
    return rays


def axis_rays(nodes, tris, seed, per_kind=40):
    """Directions with one or two zero components -- the zeros of either sign, the other components of either sign -- from origins inside
    the root box, exactly on one of its faces, and outside it.  Every second ray passes through a point of a triangle (the origin lies
    behind that point, against the direction: as far as the box goes for "face", beyond it for "outside"); the others start anywhere.
    tmin 0, tmax a twentieth, a third or three times the box diagonal."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(nodes)
    size = hi - lo
    diag = float(np.linalg.norm(size))
    org, d = [], []
    masks = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]                 # 1 = that component is zero
    count = len(masks) * 2 * 3 * per_kind
    targets = np.clip(_aim_points(nodes, tris, rng, count, (2.0, 2.0, 2.0)), lo, hi)
    for mask in masks:
        for zero in (0.0, -0.0):
            for where in ("inside", "face", "outside"):
                for j in range(per_kind):
                    dd = np.where(np.array(mask) == 1, zero, rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3))
                    free = [a for a in range(3) if not mask[a]]
                    if j % 2 == 0:
                        # back from the target until the box ends: along axis `a` first
                        t = targets[len(org)]
                        back = [((t[a] - lo[a]) if dd[a] > 0 else (hi[a] - t[a])) / abs(dd[a]) for a in free]
                        a = free[int(np.argmin(back))]
                        s = min(back) * {"inside": rng.uniform(0.1, 0.9), "face": 1.0, "outside": 1.3}[where]
                        o = t - dd * (s + (0.1 * diag if where == "outside" else 0.0))
                        if where == "face":
                            o[a] = lo[a] if dd[a] > 0 else hi[a]
                    else:
                        o = rng.uniform(lo + 0.02 * size, hi - 0.02 * size)
                        a = free[j % len(free)]
                        if where == "face":                     # on the face the ray leaves through or enters by, in turn
                            o[a] = (hi if (dd[a] > 0) == (j % 4 == 1) else lo)[a]
                        elif where == "outside":                # beside the box along a free axis, looking at it or away from it
                            side = hi[a] + 0.3 * size[a] if dd[a] < 0 else lo[a] - 0.3 * size[a]
                            o[a] = side if j % 4 == 1 else (lo[a] + hi[a]) - side
                    org.append(o); d.append(dd)
    rays = F.make_rays(np.array(org, "<f4"), np.array(d, "<f4"), 0.0, 1.0)
    rays["tmax"] = (diag * rng.choice([0.05, 0.3, 3.0], len(rays))).astype("<f4")
    return rays


def chain_rays(n, seed, jitter):
    """The rays of the chain tests (test_gpu_parity.test_deep_stacks_in_the_persistent_kernels): along +z through the chain, every third
    one beside it; jitter: no two directions alike."""
    rng = np.random.default_rng(seed)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[::3, 0] += 50.0
    d = np.tile(np.float32([0.001, 0.002, 1.0]), (n, 1))
    if jitter:
        d[:, :2] += rng.uniform(-1e-4, 1e-4, (n, 2)).astype("<f4")
    return F.make_rays(org, d, 0.0, 1000.0)


# ---- hierarchies ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cornell_bvh():
    return F.read_bvh(GOLDEN / "cornell.bvh", F.BVH2_TRI1)


@functools.lru_cache(maxsize=None)
def _soup_bvh():
    v, ix = soup_mesh()
    nodes, tris, info = lbvh_model.build(v, ix, 2)
    return nodes, tris


def _soup_ray_sets(nodes, tris):
    return {"segments": segment_rays(nodes, tris, 4096, 5), "specials": special_rays(nodes, tris, 6), "axis": axis_rays(nodes, tris, 7)}


def padding_levels(oracle):
    """Wrapper levels that bring the deepest stack of the soup's rays (closest hit) to PADDED_DEPTH_SPAN[1] entries."""
    nodes, tris = _soup_bvh()
    deepest = max(int(oracle.ray_depths(nodes, tris, r).max()) for r in _soup_ray_sets(nodes, tris).values())
    return PADDED_DEPTH_SPAN[1] - deepest


@functools.lru_cache(maxsize=None)
def _cached(name, levels):
    if name == "cornell":
        nodes, tris = _cornell_bvh()
        from conftest import GOLDEN as G
        sets = {"edge": F.read_rays(G / "cornell-edge.rays", 0.0, 100.0), "random": F.read_rays(G / "cornell-random-4096.rays", 0.0, 1.0),
                "specials": special_rays(nodes, tris, 1), "axis": axis_rays(nodes, tris, 2)}
    elif name in ("soup", "padded"):
        nodes, tris = _soup_bvh()
        sets = _soup_ray_sets(nodes, tris)                                  # the padded tree has the soup's box: the same rays
        if name == "padded":
            nodes = pad_bvh2_depth(nodes, levels)
    else:
        depth = int(name[len("chain"):])
        nodes, tris = chain_bvh2(depth)
        sets = {"chain": chain_rays(3000, depth, False), "chain_jitter": chain_rays(3000, depth + 1, True)}
    num_materials = int(tris["geom_id"].max()) + 1
    return SimpleNamespace(name=name, nodes=nodes, tris=tris, num_materials=num_materials, ray_sets=sets,
                           scene=scene_of(nodes, tris, num_materials))


def hierarchy(name, oracle=None):
    """name in HIERARCHIES -> namespace(name, nodes, tris, num_materials, scene, ray_sets {set name: Ray1 array}); "padded" needs the
    oracle (padding_levels).  Cached: nobody writes into what this returns."""
    return _cached(name, padding_levels(oracle) if name == "padded" else 0)


# ---- expected results ----------------------------------------------------------------------------------------------------------------
def geometry_of_primitive(tris):
    """geom_id of every triangle id (TRI1["prim_id"] without its end-of-leaf bit)."""
    prim = tris["prim_id"] & 0x7FFFFFFF
    out = np.full(int(prim.max()) + 1, -1, "<i4")
    out[prim] = tris["geom_id"]
    return out


def expected_records(oracle, scene, rays):
    """(geom_id, prim_id, t, u, v) of a closest-hit pass.  Hit: the hit triangle's geom_id and id, the oracle's t, u, v.  Miss:
    num_materials, -1, the ray's tmax bit for bit as given, 0, 0."""
    ref, _ = oracle.traverse(2, scene.nodes, scene.tris, rays)
    hit = ref["tri_id"] >= 0
    geom = np.where(hit, geometry_of_primitive(scene.tris)[np.where(hit, ref["tri_id"], 0)], len(scene.materials)).astype("<i4")
    prim = np.where(hit, ref["tri_id"], -1).astype("<i4")
    zero = np.float32(0.0)
    t = np.where(hit, ref["t"].view("<u4"), np.ascontiguousarray(rays["tmax"]).view("<u4")).astype("<u4").view("<f4")
    return geom, prim, t, np.where(hit, ref["u"], zero).astype("<f4"), np.where(hit, ref["v"], zero).astype("<f4")


def lit_contributions(oracle, scene, rays, ids, colours, inv_spp, n):
    """(pixel, fp32 contribution colour x inv_spp) of every shadow ray i < n with ids[i] >= 0 that nothing occludes."""
    ids = np.asarray(ids)
    live = (np.arange(len(rays)) < n) & (ids >= 0)
    occluded, _ = oracle.traverse(2, scene.nodes, scene.tris, np.ascontiguousarray(rays[live]), any_hit=True)
    lit = np.flatnonzero(live)[occluded["tri_id"] < 0]
    return ids[lit], np.asarray(colours, "<f4")[lit] * np.float32(inv_spp)


def expected_film(oracle, scene, rays, ids, colours, inv_spp, n, num_pixels=None):
    """The film (num_pixels, 3) a shadow pass adds up, in fp64, from the rays i < n with ids[i] >= 0 alone: pixel ids[i] gets
    fp32(colour x inv_spp) of every such ray the oracle finds unoccluded.  (A pixel with one contribution is exact in fp32.)"""
    pixel, c = lit_contributions(oracle, scene, rays, ids, colours, inv_spp, n)
    film = np.zeros((num_pixels if num_pixels is not None else int(np.max(ids, initial=-1)) + 1, 3), np.float64)
    np.add.at(film, pixel, c.astype(np.float64))
    return film


def film_sum_bound(oracle, scene, rays, ids, colours, inv_spp, n, num_pixels):
    """Per pixel and channel, the error bound of an fp32 sum of the pixel's k contributions in ANY order: gamma x sum |c_i| with
    gamma = (k - 1) u / (1 - (k - 1) u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    pixel, c = lit_contributions(oracle, scene, rays, ids, colours, inv_spp, n)
    k = np.bincount(pixel, minlength=num_pixels).astype(np.float64)
    total = np.zeros((num_pixels, 3), np.float64)
    np.add.at(total, pixel, np.abs(c.astype(np.float64)))
    u = 2.0 ** -24
    gamma = np.maximum(k - 1, 0) * u / (1 - np.maximum(k - 1, 0) * u)
    return gamma[:, None] * total


# ---- sizes and dead shadow rays ------------------------------------------------------------------------------------------------------
# around a wave (64 rays) and a ticket group of the persistent kernels (32 chunks = 2048 rays)
EDGE_SIZES = (1, 63, 64, 65, 2047, 2048, 2049)
# the second ticket row of k_trace_refill's index_of: 64 stripes x 2048 rays, and a wave and a ray more
SECOND_ROW_SIZE = 64 * 2048 + 65


def take(rays, n):
    """The first n rays of the set repeated as often as it takes."""
    return np.ascontiguousarray(np.resize(rays, n))


def dead_ray_ids(n):
    """Pixel ids of n shadow rays, ray i on pixel i, with dead rays (-1) between live ones: lanes 0 and 63 of every wave w with w % 8 == 1,
    the whole wave for w % 8 == 3, every second lane for w % 8 == 5, and every third lane of the last, partial wave."""
    i = np.arange(n)
    w, lane = i // 64, i % 64
    dead = ((w % 8 == 1) & ((lane == 0) | (lane == 63))) | (w % 8 == 3) | ((w % 8 == 5) & (lane % 2 == 1))
    if n % 64:
        dead |= (w == n // 64) & (lane % 3 == 0)
    return np.where(dead, -1, i).astype("<i4")


def device_sizes(n):
    """Device-side sizes of a shadow list of n rays: all of it, one less, the middle of a wave, nothing."""
    return (n, n - 1, (n // 2) // 64 * 64 + 37, 0)


def dead_case_size(oracle):
    """The smallest size above EDGE_SIZES, ending inside a wave, of the soup's segments under dead_ray_ids at which the first ray behind
    every device_sizes(n) between 0 and n is alive and unoccluded: left out by the size alone, it would show in the film if a kernel traced
    it."""
    h = hierarchy("soup")
    rays = h.ray_sets["segments"]
    occluded = oracle.traverse(2, h.nodes, h.tris, rays, any_hit=True)[0]["tri_id"] >= 0
    for n in range(max(EDGE_SIZES) + 1, len(rays)):
        ids = dead_ray_ids(n)
        if n % 64 > 1 and all(ids[size] >= 0 and not occluded[size] for size in device_sizes(n)[1:3]):
            return n
    raise AssertionError("no such size")
