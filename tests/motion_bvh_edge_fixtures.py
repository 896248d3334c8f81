"""Edge inputs for deforming meshes under motion (include/rodent_motion.h: k_fuse_motion, k_bvh2_motion): small meshes at two keys, times
and ray classes, with every expectation taken from tests/motion_bvh_model.py.  tests/test_motion_bvh_edge_fixtures.py shows on the CPU
that the inputs are not vacuous; tests/test_gpu_motion_bvh_edges.py holds the device build, the fuse and the kernel to them.

Shapes (SHAPES): `tiny1` / `tiny2` / `tiny3` (1, 2 and 3 triangles: under max_leaf 8, and `tiny1` under any, the root is ONE leaf beside
an empty slot), a seeded soup of 200 unit-size triangles as `far` (offset by 2^20, where a float's step is 1/8), `small` (scaled by
2^-20) and `huge` (scaled to 1e10), `still` (`far`'s key 0 at both keys, bit for bit) and `collapsing` (64 triangles: 16 mirrored across
their own base -- a line at t = 0.5 exactly --, 16 that shrink to a point at key 1, 16 whose winding is reversed between the keys, 16
ordinary ones).  GARBAGE: `far`'s records with the words no reader may look at set to garbage (garbage_records).
Times: the 16 of motion_bvh_fixtures.palette and the two floats beside 0.5 (7 refused, 11 traced), cycled over the rays with a shift
after every 144 (time_index): the 12 x 12 specials of class a repeat every 144 rays, and 144 is a multiple of 18.
Ray classes (CLASSES), each (rays, times): a the 12 x 12 tmin / tmax specials, b axis rays +-e_a with instance_edge_fixtures.BESIDE
pairs on the two other axes, started beside a triangle at the ray's time, c base rays as they are and with one NaN / +-inf word, d
instance_edge_fixtures.box_rays of one leaf's interpolated widened box (motion_bvh_model.at_time at D_TIMES), every ray at the time its
box was taken at, e tmax = the model's t and its two neighbours.  A ray's direction is target - origin, so a hit lies near t = 1.
"""
from __future__ import annotations

import numpy as np

import instance_edge_fixtures as E
import lbvh_model as L
import motion_bvh_fixtures as X
import motion_bvh_model as MB
from rodent_amd import formats as F

F32, F64 = np.float32, np.float64
FLT_MAX = E.FLT_MAX
HALF = F32(0.5)
BESIDE_HALF = np.array([np.nextafter(HALF, F32(0)), np.nextafter(HALF, F32(1))], F32)
OFFSET, SMALL, HUGE = 2.0 ** 20, 2.0 ** -20, 2.5e9                      # the soup's coordinates lie in (-4, 4): 4 * 2.5e9 = 1e10
SHAPES = ("tiny1", "tiny2", "tiny3", "far", "small", "huge", "still", "collapsing")
TINY = SHAPES[:3]
GARBAGE = "garbage_words"
CLASSES = "abcde"
MAX_LEAVES = {name: (1, 2, 8) if name in TINY else (2,) for name in SHAPES}
CASES = [(name, cls) for name in SHAPES for cls in CLASSES]
D_TIMES = np.array([0.0, BESIDE_HALF[1], 0.8125], F32)
W_GARBAGE, PAD_GARBAGE = np.int32(-1), np.uint32(0xDEADBEEF).view(np.int32)


# ---- times --------------------------------------------------------------------------------------------------------------------------------
def palette():
    """The 18 times: motion_bvh_fixtures.palette (7 traced fixed ones, 7 refused, 2 seeded) and the two floats beside 0.5."""
    p = np.concatenate([X.palette(), BESIDE_HALF])
    assert len(set(p.view("<u4").tolist())) == 18 and MB.traced(p).sum() == 11
    return p


def time_index(n):
    k = np.arange(n)
    return (k + 5 * (k // 144)) % 18


def times_for(n):
    return palette()[time_index(n)]


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------
def _mesh(corners):
    """(vertices (3 n, 4), indices (n, 4)) of n triangles with corners of their own; the geometry id cycles over 0 .. 4."""
    c = np.asarray(corners).reshape(-1, 3, 3)
    v = np.zeros((3 * len(c), 4), F32)
    v[:, :3] = c.reshape(-1, 3).astype(F32)
    ix = np.zeros((len(c), 4), np.int32)
    ix[:, :3] = np.arange(3 * len(c)).reshape(-1, 3)
    ix[:, 3] = np.arange(len(c)) % 5
    return v, ix


def _soup(n=200, seed=41):
    """(key 0, key 1) float64 (n, 3, 3): unit-size triangles in (-4, 4)^3, key 1 moved by up to the triangle's size per corner."""
    rng = np.random.default_rng(seed)
    k0 = rng.uniform(-3, 3, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    return k0, k0 + rng.uniform(-1, 1, (n, 3, 3))


def _collapsing(seed=43):
    rng = np.random.default_rng(seed)
    k0, k1 = np.zeros((64, 3, 3)), np.zeros((64, 3, 3))
    for i in range(64):
        centre = rng.integers(-12, 13, 3) * 0.25
        if i < 16:
            # corners on multiples of 1/4, the base along one axis: the mirror image and the midpoint of the apex are exact
            a = i % 3
            base = centre.copy()
            far_end = base.copy(); far_end[a] += 0.25 * rng.integers(2, 7)
            apex = base.copy(); apex[a] += 0.25; apex[(a + 1) % 3] += 0.25 * rng.integers(1, 6); apex[(a + 2) % 3] -= 0.25 * rng.integers(0, 4)
            mirrored = 2 * base - apex; mirrored[a] = apex[a]
            k0[i], k1[i] = (base, far_end, apex), (base, far_end, mirrored)
        else:
            k0[i] = centre + rng.uniform(-1, 1, (3, 3))
            if i < 32:
                k1[i] = k0[i].mean(0) + rng.uniform(-0.5, 0.5, 3)                   # one point
            elif i < 48:
                k1[i] = k0[i][[0, 2, 1]] + rng.uniform(-0.5, 0.5, 3)                # the other winding, moved as a whole
            else:
                k1[i] = k0[i] + rng.uniform(-1, 1, (3, 3))
    return k0, k1


class Shape:
    def __init__(self, name, k0, k1):
        self.name = name
        self.v0, self.ix = _mesh(k0)
        self.v1 = _mesh(k1)[0]
        self.n = len(self.ix)

    def corners(self, key):
        return (self.v0, self.v1)[key][:, :3].reshape(self.n, 3, 3).astype(F64)


def _shapes():
    rng = np.random.default_rng(47)
    out = {}
    for n in (1, 2, 3):
        # inside (-0.6, 0.6)^3: a ray parallel to a face of a box inside (-1, 1) is culled by its side of the face
        # (instance_edge_fixtures' docstring), not by the overflow of org * FLT_MAX
        k0 = rng.uniform(-0.1, 0.1, (n, 1, 3)) + rng.uniform(-0.35, 0.35, (n, 3, 3))
        out[f"tiny{n}"] = Shape(f"tiny{n}", k0, k0 + rng.uniform(-0.15, 0.15, (n, 3, 3)))
    k0, k1 = _soup()
    out["far"] = Shape("far", k0 + OFFSET, k1 + OFFSET)
    out["small"] = Shape("small", k0 * SMALL, k1 * SMALL)
    out["huge"] = Shape("huge", k0 * HUGE, k1 * HUGE)
    out["still"] = Shape("still", k0 + OFFSET, k0 + OFFSET)
    out["collapsing"] = Shape("collapsing", *_collapsing())
    assert out["still"].v0.tobytes() == out["still"].v1.tobytes() == out["far"].v0.tobytes()
    return out


SHAPE = _shapes()


# ---- records --------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def topology(name, max_leaf):
    """lbvh_model's tree over key 0 (the device's build_bvh2(max_leaf=...) writes the same bytes)."""
    key = ("topology", name, max_leaf)
    if key not in _cache:
        sh = SHAPE[name]
        nodes, tris, info = L.build(sh.v0, sh.ix, max_leaf)
        assert info[2] == 0
        _cache[key] = (nodes, tris)
    return _cache[key]


def records(name, max_leaf):
    """The model's motion records (mn, mt) of a shape over topology(name, max_leaf); GARBAGE: garbage_records of `far`."""
    key = ("records", name, max_leaf)
    if key not in _cache:
        if name == GARBAGE:
            _cache[key] = garbage_records(*records("far", max_leaf))
        else:
            sh = SHAPE[name]
            nodes, tris = topology(name, max_leaf)
            mn, mt, info = MB.build(nodes, tris, sh.v0, sh.v1, sh.ix)
            assert info.tolist() == [len(nodes), len(nodes) + len(tris), 0, len(nodes)], (name, info)
            _cache[key] = (mn, mt)
    return _cache[key]


def garbage_records(mn, mt):
    """The records with key 1's three w words set to 0xFFFFFFFF and a node's six pad words to 0xDEADBEEF; the child words, the bounds
    and key 0 stay as they are."""
    mn, mt = mn.copy(), mt.copy()
    mn["pad"] = PAD_GARBAGE
    key1 = mt["key1"]
    for w in MB.WORDS:
        key1[w] = W_GARBAGE
    mt["key1"] = key1
    return mn, mt


def has_empty_slot(name, max_leaf):
    return bool((topology(name, max_leaf)[0]["child"] == 0).any())


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------
def _at(sh, times):
    """(n, ntri, 3, 3) float64: every triangle at every ray's time (a refused time: clamped, the ray is a miss whatever it is)."""
    with np.errstate(invalid="ignore"):
        t = np.clip(np.nan_to_num(np.asarray(times, F64), nan=0.5), 0.0, 1.0)[:, None, None, None]
    return (1 - t) * sh.corners(0)[None] + t * sh.corners(1)[None]


def _extent(sh):
    both = np.concatenate([sh.corners(0), sh.corners(1)]).reshape(-1, 3)
    lo, hi = both.min(0), both.max(0)
    return (lo + hi) / 2, float((hi - lo).max())


def aimed(name, n, seed, times):
    """n rays aimed at a point well inside a triangle at the ray's own time, from outside the mesh (even rays) and from its middle
    (odd rays).  Every fourth ray is a miss: aimed past the mesh from outside, or ending after 2 % of its way from inside."""
    sh = SHAPE[name]
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, sh.n, n)
    c = _at(sh, times)[np.arange(n), tri]
    u, v = rng.uniform(0.15, 0.4, (2, n, 1))
    target = c[:, 0] + u * (c[:, 1] - c[:, 0]) + v * (c[:, 2] - c[:, 0])
    centre, extent = _extent(sh)
    k = np.arange(n)
    outside, past = (k % 2 == 0), (k % 4 == 3)
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    org = np.where(outside[:, None], centre + 1.5 * extent * away, centre + 0.05 * extent * away)
    target[past & outside] += 3.0 * extent * np.roll(away, 1, axis=1)[past & outside]
    tmax = np.where(past & ~outside, F32(0.02), FLT_MAX).astype(F32)
    return F.make_rays(org.astype(F32), (target - org).astype(F32), 0.0, tmax)


def class_a(name):
    n = 4 * len(E.SPECIALS) ** 2
    times = times_for(n)
    rays = aimed(name, n, 1, times)
    k = np.arange(n)
    rays["tmin"], rays["tmax"] = E.SPECIALS[k % len(E.SPECIALS)], E.SPECIALS[(k // len(E.SPECIALS)) % len(E.SPECIALS)]
    return rays, times


def class_b(name):
    """Axis rays: 6 directions x the 36 pairs of BESIDE values on the two other axes (every third ray ends at 1e-9 of its way), then 72
    rays along -e_a beside negative zeros and negative tiny values.  A ray starts half the mesh's triangle size away from a point of
    a triangle at its own time, on the side the ray comes from."""
    sh = SHAPE[name]
    rng = np.random.default_rng(2)
    n = 216 + 72
    times = times_for(n)
    axes = np.array([(r % 6) // 2 if r < 216 else (r - 216) % 3 for r in range(n)])
    # 64 candidate points per ray; the first whose coordinates on the two other axes lie inside (-0.9, 0.9) is taken (else the first)
    tri = rng.integers(0, sh.n, (n, 64))
    u, v = rng.uniform(0.2, 0.35, (2, n, 64, 1))
    c = _at(sh, times)[np.arange(n)[:, None], tri]
    points = c[:, :, 0] + u * (c[:, :, 1] - c[:, :, 0]) + v * (c[:, :, 2] - c[:, :, 0])
    other = np.abs(points) < 0.9
    other[np.arange(n), :, axes] = True
    point = points[np.arange(n), other.all(2).argmax(1)]
    size = float(np.abs(sh.corners(0) - sh.corners(0).mean(1, keepdims=True)).max())
    negative = [(-0.0, -0.0), (-0.0, -1e-9), (-1e-40, -0.0), (-0.0, -1e-40)]
    d, tmax = [], []
    for r in range(n):
        if r < 216:
            a, sign = (r % 6) // 2, 1.0 - 2.0 * (r % 2)
            pick = (r // 6 + 11 * (r % 6)) % 36
            beside = [E.BESIDE[pick % 6], E.BESIDE[pick // 6]]
            tmax.append(F32(1e-9) if r % 3 == 2 else FLT_MAX)
        else:
            a, sign, beside = (r - 216) % 3, -1.0, list(negative[((r - 216) // 3) % 4])
            tmax.append(FLT_MAX)
        d.append([sign * size if col == a else beside.pop() for col in range(3)])
    d = np.array(d, F64)
    axis = np.abs(d).argmax(1)
    org = point.copy()
    org[np.arange(n), axis] -= 0.5 * d[np.arange(n), axis]
    return F.make_rays(org.astype(F32), d.astype(F32), 0.0, np.array(tmax, F32)), times


def class_c(name):
    base_times = times_for(40)
    base = aimed(name, 40, 3, base_times)
    out, times = [], []
    for r, t in zip(base, base_times):
        out.append(r.copy())
        for field in ("org", "dir"):
            for col in range(3):
                for value in (np.nan, np.inf, -np.inf):
                    bad = r.copy(); bad[field][col] = value
                    out.append(bad)
        times += [t] * 19
    return np.array(out, F.RAY1), np.array(times, F32)


def leaf_box(name, max_leaf, t):
    """The interpolated widened box (lo_x hi_x ...) of the first leaf slot of the tree at time t: the model's own values."""
    mn, mt = records(name, max_leaf)
    node, slot = map(int, np.argwhere(mn["child"] < 0)[0])
    return MB.at_time(mn, mt, t)[0]["bounds"][node, 6 * slot: 6 * slot + 6]


def class_d(name, max_leaf):
    """(rays, times, indices of the rays parallel to a face)."""
    rays, times, graze = [], [], []
    for k, t in enumerate(D_TIMES):
        r, g = E.box_rays(leaf_box(name, max_leaf, t), seed=4 + k)
        graze.append(g + sum(len(x) for x in rays))
        rays.append(r); times.append(np.full(len(r), t, F32))
    return np.concatenate(rays), np.concatenate(times), np.concatenate(graze)


def class_e(oracle, name, max_leaf):
    times = times_for(288)
    base = aimed(name, 288, 5, times)
    hits = MB.trace(oracle, *records(name, max_leaf), base, times)
    hit = np.flatnonzero(hits["tri_id"] >= 0)[:100]
    t = hits["t"][hit]
    out = np.repeat(base[hit], 3)
    out["tmax"] = np.stack([np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))], 1).reshape(-1)
    return out, np.repeat(times[hit], 3)


def rays_of(oracle, name, cls, max_leaf=None):
    """(rays, times) of one class on one shape.  Classes d and e are made from the records of the shape's first max_leaf unless one is
    given; the rays of GARBAGE are `far`'s."""
    name = "far" if name == GARBAGE else name
    max_leaf = MAX_LEAVES[name][-1] if max_leaf is None else max_leaf
    key = ("rays", name, cls, max_leaf if cls in "de" else 0)
    if key not in _cache:
        _cache[key] = {"a": lambda: class_a(name), "b": lambda: class_b(name), "c": lambda: class_c(name),
                       "d": lambda: class_d(name, max_leaf)[:2], "e": lambda: class_e(oracle, name, max_leaf)}[cls]()
    return _cache[key]


def expect(oracle, name, max_leaf, cls, any_hit):
    """The model's hits (HIT1) for one class on one shape's records; the rays of classes d and e are those made for the last of the
    shape's max_leaf values, whichever tree is traced."""
    key = ("expect", name, max_leaf, cls, any_hit, MB.lerp, MB.traced, MB.at_time, type(oracle).__name__)
    if key not in _cache:
        rays, times = rays_of(oracle, name, cls)
        _cache[key] = MB.trace(oracle, *records(name, max_leaf), rays, times, any_hit)
    return _cache[key]


def ordinary(rays):
    """Rays a float64 reading of the geometry can judge: finite words, 0 <= tmin < tmax, no zero or tiny direction component."""
    words = np.ascontiguousarray(rays).view("<f4").reshape(len(rays), -1)
    with np.errstate(invalid="ignore"):
        return np.isfinite(words).all(1) & (rays["tmin"] >= 0) & (rays["tmin"] < rays["tmax"]) & (np.abs(rays["dir"]) >= F32(1e-8)).all(1)


# ---- the static anchor ----------------------------------------------------------------------------------------------------------------------
STATIC_LOST_CAP = 2                                                     # per class and time; see static_anchor


def static_anchor(oracle, rays, time):
    """(static hits, brute-force hits, lost) for `still` at a time of 0, 1 or -0: the oracle over the static tree (topology("still", 2),
    tight boxes), the oracle over ONE leaf of all triangles at that time, and the rays on which the two differ in t.  Equal keys at
    t = 0 or 1 give the static triangles bit for bit, so the motion trace must equal the brute force; the static tree has nothing
    that widens its boxes, and at 2^20, where the slab test's rounding is a sixteenth of a unit, it culls a few hits the brute force
    has (the same loss the model shows with the widening set to 0)."""
    from test_motion_bvh_model import single_leaf
    nodes, tris = topology("still", 2)
    at = MB.at_time(*records("still", 2), F32(time))[1]
    for name in MB.GEOMETRY:
        assert np.array_equal(at[name], tris[name])
    static = oracle.traverse(2, nodes, tris, rays)[0]
    brute = oracle.traverse(2, *single_leaf(at), rays)[0]
    return static, brute, static["t"].view("<u4") != brute["t"].view("<u4")


# ---- the named perturbations of the model ---------------------------------------------------------------------------------------------------
def fused_lerp(x0, x1, t):
    """lerp contracted as a compiler would: fma(t, x1, s * x0)."""
    t = F32(t)
    with np.errstate(all="ignore"):
        s = F32(1) - t
        return E.M.fma32(t, np.asarray(x1, F32), s * np.asarray(x0, F32))


def one_product_lerp(x0, x1, t):
    """x0 + t * (x1 - x0)."""
    x0, x1 = np.asarray(x0, F32), np.asarray(x1, F32)
    with np.errstate(all="ignore"):
        return (x0 + F32(t) * (x1 - x0)).astype(F32)


def clamped_lerp(x0, x1, t):
    with np.errstate(invalid="ignore"):
        return _LERP(x0, x1, np.clip(F32(t), F32(0), F32(1)))


_LERP, _AT_TIME = MB.lerp, MB.at_time


def _strict_one(times):
    t = np.asarray(times, F32)
    with np.errstate(invalid="ignore"):
        return (t >= 0) & (t < 1)


def _no_negative_zero(times):
    t = np.asarray(times, F32)
    with np.errstate(invalid="ignore"):
        return (t >= 0) & (t <= 1) & ~((t == 0) & np.signbit(t))


def key1_words_at_time(mn, mt, t):
    """at_time with key 1's w words in place of key 0's.  (Only for records whose key 1 words end every leaf: GARBAGE.)"""
    nodes, tris = _AT_TIME(mn, mt, t)
    for w in MB.WORDS:
        tris[w] = mt["key1"][w]
    assert (tris["prim_id"] < 0).all()
    return nodes, tris


class EmptySlotTaken:
    """oracle.binding as it would walk with the `child != 0` of the node step dropped, for ONE-node trees (every tree with an empty slot
    here is one).  The empty slot's bounds are (+inf, -inf) at both keys; interpolated they are that again, or NaN at t = 0 and t = 1
    (1 * inf + 0 * inf).  Either way every slab product is an infinity of each sign or a NaN, the minNum / maxNum of the slab test drop
    them, and the test passes whenever tmin <= tmax with an entry distance of tmin exactly -- never behind the leaf's, so the strict
    te0 < te1 walks the empty slot first: child word 0, the word that ends the traversal.  Every such ray is a miss."""

    def __init__(self, oracle):
        self.oracle = oracle

    def traverse(self, width, nodes, tris, rays, any_hit=False):
        hits, stats = self.oracle.traverse(width, nodes, tris, rays, any_hit=any_hit)
        if len(nodes) == 1 and (nodes["child"][0] == 0).any():
            with np.errstate(invalid="ignore"):
                ends = rays["tmin"] <= rays["tmax"]
            hits = hits.copy()
            hits["tri_id"][ends], hits["t"][ends], hits["u"][ends], hits["v"][ends] = -1, rays["tmax"][ends], 0, 0
        return hits, stats


def perturbations():
    """name: {attribute of motion_bvh_model: its replacement}."""
    return {"fused": {"lerp": fused_lerp},
            "one_product": {"lerp": one_product_lerp},
            "one_refused": {"traced": _strict_one},
            "negative_zero_refused": {"traced": _no_negative_zero},
            "clamped": {"traced": lambda times: ~np.isnan(np.asarray(times, F32)), "lerp": clamped_lerp},
            "key1_words": {"at_time": key1_words_at_time}}
