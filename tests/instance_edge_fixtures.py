"""Edge inputs for the instanced kernels (include/rodent_instances.h): edge matrices, top levels, ray classes and stack layouts, with
every expectation taken from tests/instance_model.py.  tests/test_instance_edge_fixtures.py shows on the CPU that the inputs are not
vacuous; tests/test_gpu_instanced_edges.py holds k_instanced and k_trace_instanced to them.

Objects: 0 = the Cornell BVH2 block (x in [-1.02, 1], y in [0, 1.99], z in [-1.04, 0.99], open towards +z), 1 = instance_model.flat_object().
Top levels (TOPS): `one` (n = 1: a scale of 1/4 near the origin, so every face of its world box lies inside (-1, 1), where a ray parallel
to a face is culled by its side of the face and not by the overflow of org * FLT_MAX), `pair` (n = 2, coincident), `stack64` (64
coincident instances: equal Morton codes, Karras splits by index alone, every te0 < te1 is a tie), `edges` (the edge-matrix set) and
`leaf8` (8 boxes in a row: one leaf of 8 under max_leaf 8).
Ray classes (CLASSES): a the 12 x 12 tmin / tmax specials, b world axis rays with {+-0, +-1e-40, +-1e-9} beside the axis, c one NaN /
+-inf word (every base ray also as it is: only those hit, a non-finite word makes every triangle test fail), d origins inside a world box,
on its widened faces and rays parallel to a face a few ulps on either side of it, e tmax = the model's t and its two neighbours, f rays
through coincident instances.  A ray aimed at an instance is made in that object's space and carried out through the fp64 matrix.
"""
from __future__ import annotations

import numpy as np

import instance_model as M
from conftest import chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

F32, F64 = np.float32, np.float64
FLT_MAX = M.FLT_MAX
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345,
                     0x40A00000, 0xBF800000, 0x3C23D70A, 0x7F7FFFFF], dtype="<u4").view("<f4")   # test_special_tmin_tmax_values'
BESIDE = np.array([0x00000000, 0x80000000], "<u4").view("<f4").tolist() + [1e-40, -1e-40, 1e-9, -1e-9]
MAX_LEAVES = (1, 2, 8)
CLASSES = {"a": ("one", "pair", "edges"), "b": ("one", "edges"), "c": ("one", "edges"), "d": ("one", "edges"),
           "e": ("one", "pair", "edges", "leaf8"), "f": ("pair", "stack64", "edges", "leaf8")}
CASES = [(top, cls) for cls, tops in CLASSES.items() for top in tops]


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------
def place(linear, translation=(0, 0, 0)):
    t = np.zeros((3, 4)); t[:, :3] = linear; t[:, 3] = translation
    return t.reshape(12).astype(F32)


def _rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


RX90, RY90, RZ90 = [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
QUARTER = place(np.eye(3) * 0.25, (0.25, -0.5, 0.25))
COINCIDENT = place(_rot_y(0.5) * 0.75, (0.5, 0.25, -0.5))
# Rows 0 and 1 differ in bit 3 of one entry; the inverse's entries are 2^20 + 1 and +-2^20, so a rounding error of a world coordinate
# comes back a million times larger.  It is placed at (0, 0, -16) and its rays are made of multiples of 1/4 (_dyadic_object_space): then
# the world ray, every product and every sum of the object-space ray are exact, and the model can be checked against float64.
NEAR_SINGULAR = [[1, 1, 0], [1, 1 + 2.0 ** -20, 0], [0, 0, 1]]
_cell = lambda k: (8.0 * (k % 5), 0.0, -8.0 * (k // 5))


def edge_matrices():
    """[(name, matrix (12,) float32, object)]: every placement is accepted by instance_model.invert.  The 2^20 scale is placed so that
    the whole small layout lies in the air of its box (object-space (-0.5, 1.5, 0.25)): every ray enters it, short ones leave it alone."""
    named = [("quarter", QUARTER, 0), ("identity", place(np.eye(3), _cell(1)), 0)]
    for k, (name, lin) in enumerate((("rx90", RX90), ("ry90", RY90), ("rz90", RZ90), ("rx180", np.diag([1, -1, -1])),
                                     ("ry180", np.diag([-1, 1, -1])), ("rz180", np.diag([-1, -1, 1])),
                                     ("permutation", [[0, 0, 1], [1, 0, 0], [0, 1, 0]]), ("mirror", np.diag([-1, 1, 1])))):
        named.append((name, place(lin, _cell(2 + k)), 0))
    named += [("scale_2^-20", place(np.eye(3) * 2.0 ** -20, _cell(13)), 0),
              ("scale_2^20", place(np.eye(3) * 2.0 ** 20, (2.0 ** 19, -3 * 2.0 ** 19, -2.0 ** 18)), 0),
              ("non_uniform", place(np.diag([1e-3, 1e3, 1.0]), _cell(11)), 0),
              ("shear", place([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1]], _cell(12)), 0),
              ("near_singular", place(NEAR_SINGULAR, _cell(10)), 0),
              ("translation_2^20", place(np.eye(3), (2.0 ** 20, 0, 0)), 0),
              ("coincident_0", COINCIDENT + place(np.zeros((3, 3)), _cell(14)), 0),
              ("coincident_1", COINCIDENT + place(np.zeros((3, 3)), _cell(14)), 0),
              ("flat_axis_aligned", place(np.diag([1.5, 0.75, 2.0]), _cell(15)), 1)]
    return named


AXIS_ALIGNED = ("quarter", "identity", "rx90", "ry90", "rz90", "rx180", "ry180", "rz180", "permutation", "mirror", "scale_2^-20",
                "scale_2^20", "non_uniform", "translation_2^20", "flat_axis_aligned")
FLAG_BOUNDARY = {-127: 0, -128: M.BAD_TRANSFORM}                        # uniform scale 2^k: the inverse 2^127 is finite, 2^128 is not


class Top:
    """A top level: transforms (n, 12), object ids, instance ids, the instances rays are aimed at, and those with axis-aligned matrices."""

    def __init__(self, name, transforms, obj, aimed, axis):
        self.name, self.transforms, self.obj = name, np.asarray(transforms, F32).reshape(-1, 12), np.asarray(obj, np.int32)
        self.n = len(self.obj)
        self.ids = (np.arange(self.n) * 5 + 2).astype(np.int64)
        self.aimed, self.axis = list(aimed), list(axis)


def _tops():
    named = edge_matrices()
    names = [n for n, _, _ in named]
    row = [place(_rot_y(0.2 * k) * (0.6 + 0.05 * k), (3.0 * k, 0.1 * k, 0.5 * (k % 3))) for k in range(8)]
    return {"one": Top("one", [QUARTER], [0], [0], [0]),
            "pair": Top("pair", [COINCIDENT] * 2, [0, 0], [0], []),
            "stack64": Top("stack64", [COINCIDENT] * 64, [0] * 64, [0], []),
            "edges": Top("edges", [m for _, m, _ in named], [o for _, _, o in named], range(len(named)),
                         [names.index(n) for n in AXIS_ALIGNED]),
            "leaf8": Top("leaf8", row, [0] * 8, range(8), [])}


TOPS = _tops()


class Scene:
    """The model's side of (top level, max_leaf): the packed objects, the descriptors and the TLAS."""

    def __init__(self, block, top, max_leaf):
        self.top, self.max_leaf = top, max_leaf
        self.pairs = [block, M.flat_object()]
        self.nodes, self.tris, self.table = M.pack(self.pairs)
        self.descs = M.descriptors(top.transforms, top.obj, top.ids)
        self.tlas, self.inst, self.info = M.build_tlas(self.nodes, self.table, self.descs, max_leaf)
        self.slot = np.zeros(int(top.ids.max()) + 1, np.int64)           # instance id -> leaf-order slot
        self.slot[self.inst["instance_id"] & 0x7FFFFFFF] = np.arange(top.n)

    def model(self):
        return self.tlas, self.inst, self.nodes, self.tris

    def object_boxes(self):
        roots = self.nodes[self.table["node_offset"][self.top.obj]]
        lo, hi = zip(*(M.object_box(r) for r in roots))
        return np.array(lo), np.array(hi)

    def world_boxes(self):
        return M.world_box(self.top.transforms, *self.object_boxes())


_cache = {}


def scene(block, top, max_leaf=1) -> Scene:
    key = ("scene", top, max_leaf)
    if key not in _cache:
        _cache[key] = Scene(block, TOPS[top], max_leaf)
    return _cache[key]


# ---- rays -------------------------------------------------------------------------------------------------------------------------------
def _object_space(rng, n, obj):
    """n rays in an object's own space towards points inside it.  The Cornell block holds the front face of its tall box and a side
    face of its short box twice (equal t in two triangles), so its rays start where neither face is seen: in the air of the back right
    corner (odd rays) and outside behind that corner, through the walls (even rays).  Every fourth ray is a miss: aimed over the object
    from outside, or ending at t = 0.05 from inside."""
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    k = np.arange(n)
    past = k % 4 == 3
    tmax = np.full(n, FLT_MAX, F32)
    if obj == 0:
        outside = (k % 2 == 0)[:, None]
        org = np.where(outside, np.stack([u(1.6, 2.0), u(0.7, 1.3), u(-2.1, -1.7)], 1), np.stack([u(0.5, 0.7), u(0.8, 1.2), u(-0.9, -0.7)], 1))
        target = np.stack([u(-0.95, 0.95), u(0.05, 1.9), u(-1.0, 0.9)], 1)
        target[past & outside[:, 0]] += np.array([0.0, 6.0, 0.0])
        tmax[past & ~outside[:, 0]] = 0.05
    else:
        org = np.stack([u(-0.5, 0.5), u(-0.5, 0.5), np.full(n, 3.0)], 1)
        target = np.stack([u(-0.9, 0.9), u(-0.9, 0.9), np.full(n, 0.5)], 1)
        target[past] += np.array([4.0, 0.0, 0.0])
        tmax[past] = 2.0
    return org, target - org, tmax


def _dyadic_object_space(rng, n):
    """_object_space for the Cornell block with every origin and direction word a multiple of 1/4."""
    k = np.arange(n)
    outside = (k % 2 == 0)[:, None]
    org = np.where(outside, np.array([1.75, 1.0, -1.75]), np.array([0.5, 1.0, -0.75]))
    target = np.stack([rng.integers(-3, 4, n), rng.integers(1, 8, n), rng.integers(-3, 4, n)], 1) * 0.25
    past = k % 4 == 3
    target[past & outside[:, 0]] += np.array([0.0, 6.0, 0.0])
    tmax = np.full(n, FLT_MAX, F32)
    tmax[past & ~outside[:, 0]] = 0.05
    return org, target - org, tmax


def aimed(top, n, seed, targets=None):
    """n world rays, ray k aimed at instance targets[k % len] (default: top.aimed): made in object space, carried out through the fp64
    matrix."""
    rng = np.random.default_rng(seed)
    t = TOPS[top]
    targets = t.aimed if targets is None else targets
    org, d, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, F32)
    for j, k in enumerate(targets):
        sel = np.arange(j, n, len(targets))
        m = t.transforms[k].reshape(3, 4).astype(F64)
        exact = np.array_equal(m[:, :3], np.asarray(NEAR_SINGULAR, F32))
        o, dd, tm = _dyadic_object_space(rng, len(sel)) if exact else _object_space(rng, len(sel), int(t.obj[k]))
        org[sel], d[sel], tmax[sel] = o @ m[:, :3].T + m[:, 3], dd @ m[:, :3].T, tm
    return F.make_rays(org.astype(F32), d.astype(F32), 0.0, tmax)


def class_a(top):
    rays = aimed(top, 4 * len(SPECIALS) ** 2, 1)
    k = np.arange(len(rays))
    rays["tmin"], rays["tmax"] = SPECIALS[k % len(SPECIALS)], SPECIALS[(k // len(SPECIALS)) % len(SPECIALS)]
    return rays


def class_b(top):
    """Per axis-aligned instance: world axis directions +-e_a with pairs of BESIDE values on the two other axes (`one`: all 36 pairs for
    each of the 6 directions, every third ray ending at 1e-9, before any wall), then rays along -e_a with negative zeros and negative
    tiny values beside it, which is how a sum of three products comes out as -0.  They start in the air of the object at coordinates
    inside (-1, 1): beside a zero or tiny component, inv_org = -(org * +-FLT_MAX) must stay finite for a box test to pass at all."""
    t = TOPS[top]
    org, d, tmax = [], [], []
    general = max(24, 216 // len(t.axis))
    negative = [(-0.0, -0.0), (-0.0, -1e-9), (-1e-40, -0.0), (-0.0, -1e-40)]
    for j, k in enumerate(t.axis):
        m = t.transforms[k].reshape(3, 4).astype(F64)
        inside = np.array([0.45, 0.9, 0.5]) if t.obj[k] == 0 else np.array([0.3, 0.2, 0.9])
        for r in range(general + 12):
            if r < general:
                a, sign = (r % 6) // 2, 1.0 - 2.0 * (r % 2)
                pick = (r // 6 + 11 * (r % 6) + 5 * j) % 36
                v = [BESIDE[pick % 6], BESIDE[pick // 6]]
                tmax.append(F32(1e-9) if r % 3 == 2 else FLT_MAX)
            else:
                a, sign, v = (r - general) % 3, -1.0, list(negative[(r - general) // 3])
                tmax.append(FLT_MAX)
            d.append([sign if c == a else v.pop() for c in range(3)])
            org.append((inside + 0.01 * np.array([r % 5, r % 3, r % 7])) @ m[:, :3].T + m[:, 3])
    return F.make_rays(np.array(org).astype(F32), np.array(d, F64).astype(F32), 0.0, np.array(tmax, F32))


def class_c(top):
    base = aimed(top, 24, 3)
    out = []
    for r in base:
        out.append(r.copy())
        for field in ("org", "dir"):
            for c in range(3):
                for value in (np.nan, np.inf, -np.inf):
                    bad = r.copy(); bad[field][c] = value
                    out.append(bad)
    return np.array(out, F.RAY1)


def non_finite(rays):
    """Rays with a NaN in any input word, and rays with a NaN or an infinity in an origin or direction word: chosen by the input bits."""
    words = np.ascontiguousarray(rays).view("<f4").reshape(len(rays), -1)
    geometry = np.concatenate([rays["org"], rays["dir"]], 1)
    return np.isnan(words).any(1), ~np.isfinite(geometry).all(1)


def box_rays(box, seed=4):
    """(rays, indices of the face rays) for one widened world box (lo_x hi_x lo_y hi_y lo_z hi_z, the model's own values): 128 origins
    inside it with random directions (every fourth ends at 1e-9), 48 origins exactly on its faces (tmin = 1e-3: a wall of the object
    lies within the widening, ~ 2e-7, of most faces; from 1e-3 on, what such a ray hits lies across the box), and 168 rays parallel to
    a face: along one axis with +0 / -0 on the two others, the coordinate across the face -3 ... +3 ulps from the face value, started
    outside the box along the axis.  The box must lie inside (-1, 1): see the module's docstring."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, F32)
    lo, hi = box[0::2], box[1::2]
    mid, half = (lo.astype(F64) + hi) / 2, (hi.astype(F64) - lo) / 2
    org = [mid + half * rng.uniform(-0.9, 0.9, 3) for _ in range(128)]
    d = list(rng.normal(size=(128, 3)))
    tmax = [F32(1e-9) if k % 4 == 3 else FLT_MAX for k in range(128)]
    for face in range(6):
        a, side = face // 2, face % 2
        for k in range(8):
            o = mid + half * rng.uniform(-0.9, 0.9, 3)
            o[a] = box[2 * a + side]
            v = rng.normal(size=3)
            v[a] = (abs(v[a]), -abs(v[a]), 0.0, 0.0)[k % 4] * (1 - 2 * side)       # inwards, outwards, along the face
            org.append(o); d.append(v); tmax.append(FLT_MAX)
    on_face = np.arange(128, len(org))
    graze = len(org)
    for face in range(6):
        b, side = face // 2, face % 2
        for a in ((b + 1) % 3, (b + 2) % 3):
            for ulps in range(-3, 4):
                for zero in (0.0, -0.0):
                    o = mid + half * np.array([0.31, -0.23, 0.17])
                    value = box[2 * b + side]
                    for _ in range(abs(ulps)):
                        value = np.nextafter(value, F32(np.inf if ulps > 0 else -np.inf))
                    o[b], o[a] = value, lo[a] - 0.5 * max(half[a], 0.05)
                    v = np.full(3, zero); v[a] = 1.0
                    org.append(o); d.append(v); tmax.append(FLT_MAX)
    rays = F.make_rays(np.array(org).astype(F32), np.array(d).astype(F32), 0.0, np.array(tmax, F32))
    rays["tmin"][on_face] = F32(1e-3)
    return rays, np.arange(graze, len(rays))


def class_d(block, top):
    """box_rays for the instance `quarter` (instance 0 of `one` and of `edges`)."""
    return box_rays(scene(block, top).world_boxes()[0])


def class_e(oracle, block, top):
    """tmax = the model's closest t, bit for bit, and the floats on either side of it, for 100 rays that hit."""
    base = aimed(top, 160, 5)
    hits, _ = M.trace(oracle, *scene(block, top).model(), base)
    base, t = base[hits["tri_id"] >= 0][:100], hits["t"][hits["tri_id"] >= 0][:100]
    out = np.repeat(base, 3)
    out["tmax"] = np.stack([np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))], 1).reshape(-1)
    return out


def class_f(top):
    """Rays through coincident instances: the tops that are coincident throughout, the pair of the edge set, and all of `leaf8`."""
    pair = [k for k, (name, _, _) in enumerate(edge_matrices()) if name.startswith("coincident")]
    return aimed(top, 192, 6, pair[:1] if top == "edges" else None)


def rays_of(oracle, block, top, cls):
    key = ("rays", top, cls)
    if key not in _cache:
        _cache[key] = {"a": lambda: class_a(top), "b": lambda: class_b(top), "c": lambda: class_c(top),
                       "d": lambda: class_d(block, top)[0], "e": lambda: class_e(oracle, block, top), "f": lambda: class_f(top)}[cls]()
    return _cache[key]


def expect(oracle, block, top, max_leaf, cls, any_hit):
    """(hits HIT1, instance ids) of the model for one ray class on one top level."""
    key = ("expect", top, max_leaf, cls, any_hit, M._object_rays, M.make_ray, M._instance_tmax, M._child0_first, M._miss_t)
    if key not in _cache:
        _cache[key] = M.trace(oracle, *scene(block, top, max_leaf).model(), rays_of(oracle, block, top, cls), any_hit)
    return _cache[key]


class Recorder:
    """oracle.binding with every instance the model enters written down: (object-space direction, whether a triangle was accepted, object-space origin)."""

    def __init__(self, oracle):
        self.oracle, self.calls = oracle, []

    def traverse(self, width, nodes, tris, ray, any_hit=False):
        out = self.oracle.traverse(width, nodes, tris, ray, any_hit=any_hit)
        self.calls.append((ray["dir"][0].copy(), bool(out[0][0]["tri_id"] >= 0), ray["org"][0].copy()))
        return out


def entered(oracle, sc, rays, any_hit=False):
    """Per ray the instances the model enters, in order: [(dir', accepted, org')]; none for a ray the TLAS culls everywhere.
    sc: a Scene, or the model's (tlas, instances, nodes, tris)."""
    rec, out = Recorder(oracle), []
    model = sc.model() if hasattr(sc, "model") else sc
    for k in range(len(rays)):
        rec.calls = []
        M.trace(rec, *model, rays[k:k + 1], any_hit)
        out.append(rec.calls)
    return out


# ---- the renderer's scene (instanced_scene_model: the Cornell box, a cube [-0.5, 0.5]^3 four times, an emissive quad in y = 0 twice) -------------
SCENE_OBJECT_IDS = (0, 1, 1, 1, 1, 2, 2)                                # instanced_scene_model.placements'
SCENE_BOX_TARGET = {"aligned": 6, "scaled": 1, "turned": 6}           # per matrix set the instance whose world box lies inside (-1, 1)
SCENE_CLASSES = "abcdef"


def scene_matrix_sets():
    """Three sets of 7 edge matrices for the scene's instances: between them every class of edge_matrices, the box and a quad (the
    objects with lights) at the scales 2^20 and 2^-20, and in every set instances near the origin, where axis rays can enter a box."""
    p, eye = place, np.eye(3)
    a = [p(eye), p(RZ90, (3, 0.5, 0)), p(np.diag([-1, 1, 1]), (-3, 0.5, 0)), p(_rot_y(0.5) * 0.75, (0, 3, 0)),
         p(_rot_y(0.5) * 0.75, (0, 3, 0)), p(np.diag([1.5, 0.75, 2.0]), (0, 5, 0)), p([[0, 0, 1], [1, 0, 0], [0, 1, 0]], (0.25, 0.25, -0.25))]
    b = [p(eye * 2.0 ** 20, (2.0 ** 19, -3 * 2.0 ** 19, -2.0 ** 18)), p(eye * 2.0 ** -20, (0.25, 0.5, 0.25)),
         p(np.diag([1e-3, 1e3, 1.0]), (4, 0, 0)), p([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1]], (-4, 0, 0)), p(NEAR_SINGULAR, (0, 0, -16)),
         p(eye * 2.0 ** -20, (0.5, -0.25, 0.5)), p(eye, (2.0 ** 20, 0, 0))]
    c = [p(np.diag([-1, 1, -1])), p(RX90, (3, 0.5, 0)), p(RY90, (-3, 0.5, 0)), p(np.diag([1, -1, -1]), (0, 3, 0)),
         p(np.diag([-1, -1, 1]), (0, -3, 0)), p(RZ90, (0, 5, 0)), p(eye * 0.25, (0.25, -0.5, 0.25))]
    return {"aligned": np.array(a), "scaled": np.array(b), "turned": np.array(c)}


def scene_object_rays(rng, n, obj):
    """_object_space for the scene's objects."""
    if obj == 0:
        return _object_space(rng, n, 0)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    past = np.arange(n) % 4 == 3
    if obj == 1:
        org, target = np.stack([u(-0.3, 0.3), u(-0.3, 0.3), np.full(n, 2.0)], 1), np.stack([u(-0.45, 0.45)] * 3, 1)
        target[past] += np.array([3.0, 0.0, 0.0])
    else:
        org = np.stack([u(-0.2, 0.2), np.full(n, 1.5), u(-0.2, 0.2)], 1)
        target = np.stack([u(-0.45, 0.45), np.zeros(n), u(-0.45, 0.45)], 1)
        target[past] += np.array([2.0, 0.0, 0.0])
    return org, target - org, np.where(past, F32(2.0), FLT_MAX).astype(F32)


def scene_target_box(name, transforms, model):
    """The model's widened world box of the set's box target (SCENE_BOX_TARGET)."""
    _, inst, nodes, _ = model
    k = SCENE_BOX_TARGET[name]
    slot = int(np.flatnonzero((inst["instance_id"] & 0x7FFFFFFF) == k)[0])
    lo, hi = M.object_box(nodes[inst["node_offset"][slot]])
    return M.world_box(transforms[k], lo[None], hi[None])[0]


def scene_edge_rays(oracle, name, transforms, model):
    """{class: rays} over the scene under matrix set `name` (model: (tlas, instances, nodes, tris) of that set): a the specials, b axis
    rays from a point in the air of every instance (24 + 12 as in class_b), c 28 base rays as they are and with one non-finite word, d box_rays of the
    set's box target, e tmax around the model's t, f the coincident pair (`aligned`; elsewhere: instance 3 alone)."""
    rng = np.random.default_rng(7)
    t64 = np.asarray(transforms).reshape(-1, 3, 4).astype(F64)
    ids = SCENE_OBJECT_IDS

    def to(targets, n):
        org, d, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, F32)
        for j, k in enumerate(targets):
            sel = np.arange(j, n, len(targets))
            o, dd, tm = scene_object_rays(rng, len(sel), ids[k])
            org[sel], d[sel], tmax[sel] = o @ t64[k, :, :3].T + t64[k, :, 3], dd @ t64[k, :, :3].T, tm
        return F.make_rays(org.astype(F32), d.astype(F32), 0.0, tmax)
    out = {}
    a = to(range(7), 4 * len(SPECIALS) ** 2)
    k = np.arange(len(a))
    a["tmin"], a["tmax"] = SPECIALS[k % len(SPECIALS)], SPECIALS[(k // len(SPECIALS)) % len(SPECIALS)]
    out["a"] = a
    org, d, tmax = [], [], []
    inside = {0: (0.45, 0.9, 0.5), 1: (0.1, 0.2, 0.15), 2: (0.1, 0.4, 0.2)}
    negative = [(-0.0, -0.0), (-0.0, -1e-9), (-1e-40, -0.0), (-0.0, -1e-40)]
    for j in range(7):
        for r in range(36):
            if r < 24:
                axis, sign = (r % 6) // 2, 1.0 - 2.0 * (r % 2)
                pick = (r // 6 + 11 * (r % 6) + 5 * j) % 36
                v = [BESIDE[pick % 6], BESIDE[pick // 6]]
                tmax.append(F32(1e-9) if r % 3 == 2 else FLT_MAX)
            else:
                axis, sign, v = (r - 24) % 3, -1.0, list(negative[(r - 24) // 3])
                tmax.append(FLT_MAX)
            d.append([sign if c == axis else v.pop() for c in range(3)])
            org.append(np.array(inside[ids[j]]) @ t64[j, :, :3].T + t64[j, :, 3])
    out["b"] = F.make_rays(np.array(org).astype(F32), np.array(d, F64).astype(F32), 0.0, np.array(tmax, F32))
    c = []
    for ray in to(range(7), 28):
        c.append(ray.copy())
        for field in ("org", "dir"):
            for word in range(3):
                for value in (np.nan, np.inf, -np.inf):
                    bad = ray.copy(); bad[field][word] = value
                    c.append(bad)
    out["c"] = np.array(c, F.RAY1)
    out["d"], graze = box_rays(scene_target_box(name, np.asarray(transforms, F32).reshape(-1, 12), model))
    base = to(range(7), 112)
    hits, _ = M.trace(oracle, *model, base)
    hit = hits["tri_id"] >= 0
    e = np.repeat(base[hit][:60], 3)
    t = hits["t"][hit][:60]
    e["tmax"] = np.stack([np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))], 1).reshape(-1)
    out["e"] = e
    out["f"] = to([3], 64)
    return out, graze


# ---- stack layouts ----------------------------------------------------------------------------------------------------------------------
IDENTITY = place(np.eye(3))
STACK_LAYOUTS = {                      # name: (object, TLAS padding levels, whether the launch raises the flag)
    "leaf_62": ("flat", 62, False),    # P + 2 == 64
    "leaf_63": ("flat", 63, True),     # the push of the object's end word
    "leaf_64": ("flat", 64, True),     # the push inside a TLAS step
    "chain_22": ("chain", 22, False),  # 22 + 40 + 2 == 64
    "chain_23": ("chain", 23, True),   # a push inside the object
}


def stack_layout(name):
    """(object pair, tlas nodes, instances, rays): one identity instance under a padded single-leaf TLAS; three of four rays enter the
    scene box, the others pass 50 units beside it (P = 0)."""
    what, levels, _ = STACK_LAYOUTS[name]
    obj = M.flat_object() if what == "flat" else chain_bvh2(40)
    nodes, tris, table = M.pack([obj])
    root, inst, info = M.build_tlas(nodes, table, M.descriptors(IDENTITY[None], [0], [9]), 1)
    assert info[2] == 0
    rng = np.random.default_rng(levels)
    n = 130
    org = np.zeros((n, 3), "<f4")
    org[:, :2] = rng.uniform(-0.9, 0.9, (n, 2)) if what == "flat" else rng.uniform(-4, 4, (n, 2))
    org[:, 2] = 3.0 if what == "flat" else -1.0
    org[3::4, 0] += 50.0
    d = np.float32([0.001, 0.002, -1.0 if what == "flat" else 1.0])
    return obj, pad_bvh2_depth(root, levels), inst, F.make_rays(org, np.tile(d, (n, 1)), 0.0, 1000.0)


# ---- the named perturbations of the model (tests/test_instance_edge_fixtures.py: the expectations notice each of them) --------------------
def fused_object_rays(inst, rays):
    """_object_rays with the sums contracted as a compiler would: fma(w2, z, fma(w0, x, w1 * y)) (+ w3)."""
    w = inst["world_to_object"].reshape(1, len(inst), 3, 4)
    o, d = rays["org"][:, None, :], rays["dir"][:, None, :]
    with np.errstate(all="ignore"):
        org = M.fma32(w[..., 2], o[..., 2:3], M.fma32(w[..., 0], o[..., 0:1], w[..., 1] * o[..., 1:2])) + w[..., 3]
        direction = M.fma32(w[..., 2], d[..., 2:3], M.fma32(w[..., 0], d[..., 0:1], w[..., 1] * d[..., 1:2]))
    return org.astype(F32), direction.astype(F32)


def unsigned_make_ray(org, direction):
    """make_ray with the copysign dropped: a tiny or zero component of either sign gives +FLT_MAX."""
    with np.errstate(all="ignore"):
        tiny = np.abs(direction) < F32(1e-8)
        idir = np.where(tiny, FLT_MAX, F32(1) / np.where(tiny, F32(1), direction)).astype(F32)
        return idir, -(org * idir)


def _quiet(x):
    bits = np.float32(x).view("<u4")
    return (bits | np.uint32(0x00400000)).view("<f4") if np.isnan(x) else x


def perturbations():
    """name: (attribute of instance_model, its replacement)."""
    return {"fused": ("_object_rays", fused_object_rays),
            "copysign": ("make_ray", unsigned_make_ray),
            "strict_accept": ("_instance_tmax", lambda tmax, hit_inst: F32(tmax) if hit_inst < 0 else np.nextafter(F32(tmax), F32(-np.inf))),
            "near_child_le": ("_child0_first", lambda entry0, entry1: entry0 <= entry1),
            "quiet_nan": ("_miss_t", _quiet)}
