"""Edge inputs for moving instances (the section "moving instances" of include/rodent_instances.h: the motion stage of build_tlas.h,
k_instanced_motion): motion top levels, times, ray classes and stack layouts, with every expectation taken from
tests/motion_instance_model.py.  tests/test_motion_instance_edge_fixtures.py shows on the CPU that the inputs are not vacuous;
tests/test_gpu_motion_instanced_edges.py holds build_motion_tlas and the kernel to them.  Matrices, ray makers and stack objects are
those of tests/instance_edge_fixtures.py (E): objects 0 = the Cornell BVH2 block, 1 = instance_model.flat_object().

Motion tops (TOPS), each two sets of matrices, object ids and instance ids; every endpoint is accepted by instance_model.invert:
  static_pairs  every matrix of E.edge_matrices() with M1 bitwise equal to M0
  edge_pairs    edge matrices moving to one another (EDGE_PAIRS: identity <-> 2^20 scale, 2^-20 <-> 2^20, translation 0 -> 2^20 -> `identity`,
                rx90 <-> rz90, shear <-> mirror, NEAR_SINGULAR <-> its transpose among them); instance 0 is `quarter` moving by 1/8, its
                motion box inside (-1, 1)
  crossing      diagonal pairs whose interpolation is singular strictly inside (0, 1): `flip_x` and `flip_all` exactly at 0.5 (one axis,
                all three axes change sign), `between` at a time that is no float -- its x entry is 2^-26 at 0.5 and negative at the next
                float, never 0 --, `overflow`, whose x entry is so small that the fp32 inverse is finite at the float above 0.5 and not at
                the one below (OVERFLOW_SCALE, found by overflow_scale() from the model)
  coincident    two instances with one pair of placements;  leaf8: E's row of 8, each moving
Times: motion_instance_fixtures.palette (16) and +inf, -inf, -0, nextafter(1, 2), -2^-149 and the two floats beside 0.5: 23 values,
cycled over the rays (23 is prime: every position of every class pattern meets every time).
Ray classes a - f as in E, an aimed ray carried out of object space through M(t) at its OWN time (the fp32 interpolation taken to
float64; a non-finite M(t): through M0).  Class d takes the model's motion box of instance 0.
"""
from __future__ import annotations

import numpy as np

import instance_edge_fixtures as E
import instance_model as M
import motion_instance_fixtures as X
import motion_instance_model as MM
from conftest import chain_bvh2, pad_bvh2_depth
from rodent_amd import formats as F

F32, F64 = np.float32, np.float64
FLT_MAX = E.FLT_MAX
HALF = F32(0.5)
BESIDE_HALF = np.array([np.nextafter(HALF, F32(0)), np.nextafter(HALF, F32(1))], F32)
EXTRA_TIMES = np.concatenate([F32([np.inf, -np.inf, -0.0, np.nextafter(F32(1), F32(2)), -(2.0 ** -149)]), BESIDE_HALF])
MAX_LEAVES = E.MAX_LEAVES
CLASSES = {"a": ("static_pairs", "edge_pairs", "crossing", "coincident"), "b": ("static_pairs", "edge_pairs", "crossing"),
           "c": ("static_pairs", "edge_pairs", "crossing"), "d": ("static_pairs", "edge_pairs"),
           "e": ("static_pairs", "edge_pairs", "crossing", "coincident", "leaf8"), "f": ("static_pairs", "coincident", "leaf8")}
CASES = [(top, cls) for cls, tops in CLASSES.items() for top in tops]
# (M0, M1) by the names of E.edge_matrices(); `origin` is the identity at the origin.  M1 keeps M0's place unless it is a translation pair.
EDGE_PAIRS = [("quarter", "quarter"), ("identity", "scale_2^20"), ("scale_2^20", "identity"), ("scale_2^-20", "scale_2^20"),
              ("scale_2^20", "scale_2^-20"), ("origin", "translation_2^20"), ("translation_2^20", "identity"), ("rx90", "rz90"),
              ("rz90", "rx90"), ("shear", "mirror"), ("mirror", "shear"), ("near_singular", "near_singular^T"),
              ("near_singular^T", "near_singular"), ("ry90", "permutation"), ("rx180", "ry180"), ("rz180", "non_uniform"),
              ("non_uniform", "identity"), ("permutation", "ry180"), ("ry180", "rz180"), ("coincident_0", "coincident_1")]
# No two pairs may coincide, or nearly, at any one time: the float64 brute force leaves out a ray whose two nearest candidates lie
# within 1e-4 of each other, and a pair and its reverse placed in one spot are the same instance at t = 0.5 (and four pairs that
# pass through the 2^20 scale about one point are the same huge box, to 1e-5, at every time).  So each pair through the 2^20 scale
# has an air point of its own -- the object-space point that stays where the small layout is, E's (-0.5, 1.5, 0.25) and three more
# above both boxes of the block --, the translation pair comes back to `identity`'s place and not to the origin, and the transpose of
# NEAR_SINGULAR (the matrix is symmetric: by value the same placement) stands in a place of its own, (0, 0, -32).
AIR_POINTS = {1: (-0.5, 1.5, 0.25), 2: (-0.375, 1.625, 0.375), 3: (-0.625, 1.375, 0.125), 4: (-0.25, 1.75, 0.5)}
C_SEED = 4                # class c's seed, chosen like D_SEED
D_SEED = 18               # E.box_rays' seed for class d: one for which the float64 brute force leaves out at most 2 % of its ordinary rays
DIAGONAL_PAIRS = (0, 1, 2, 3, 4, 5, 6)                                   # the pairs of EDGE_PAIRS that stay axis-aligned at every time


def palette():
    p = np.concatenate([X.palette(), EXTRA_TIMES])
    assert len(set(p.view("<u4").tolist())) == 23
    return p


def times_for(n):
    return palette()[np.arange(n) % 23]


# ---- the motion tops ------------------------------------------------------------------------------------------------------------------------
def _diag(x, y, z, translation):
    return E.place(np.diag([x, y, z]).astype(F64), translation)


def overflow_scale():
    """The x scale a = 1.5 * 2^k, k as large as possible, for which diag(a, 1/2, 1/2) -> diag(-a, 1/2, 1/2) has a non-finite fp32
    inverse at the float below 0.5 and a finite one at the float above (the step of the floats doubles at 0.5, so |s - t| does)."""
    for k in range(-90, -140, -1):
        a = 1.5 * 2.0 ** k
        bad = [M.invert(MM.lerp(_diag(a, 0.5, 0.5, (0, 0, 0)), _diag(-a, 0.5, 0.5, (0, 0, 0)), t))[1][0] for t in BESIDE_HALF]
        if bad == [True, False]:
            return a
    raise AssertionError("no such scale")


OVERFLOW_SCALE = overflow_scale()
CROSSING = {"flip_x": (_diag(0.5, 0.5, 0.5, (0, 0, 0)), _diag(-0.5, 0.5, 0.5, (0, 0, 0))),
            "flip_all": (_diag(0.5, 0.5, 0.5, (4, 0, 0)), _diag(-0.5, -0.5, -0.5, (4, 1, 0))),
            "between": (_diag(0.5, 0.5, 0.5, (0, 0, -4)), _diag(-float(np.nextafter(HALF, F32(0))), 0.5, 0.5, (0, 0, -4))),
            "overflow": (_diag(OVERFLOW_SCALE, 0.5, 0.5, (0, 0, -8)), _diag(-OVERFLOW_SCALE, 0.5, 0.5, (0, 0, -8)))}


class Top:
    """A motion top level: both sets of transforms (n, 12), object ids, instance ids, the instances rays are aimed at and those whose
    placement is axis-aligned at every time."""

    def __init__(self, name, t0, t1, obj, aimed, axis):
        self.name, self.obj = name, np.asarray(obj, np.int32)
        self.t0, self.t1 = (np.asarray(t, F32).reshape(-1, 12) for t in (t0, t1))
        self.n = len(self.obj)
        self.ids = (np.arange(self.n) * 5 + 2).astype(np.int64)
        self.aimed, self.axis = list(aimed), list(axis)
        assert not M.invert(self.t0)[1].any() and not M.invert(self.t1)[1].any()

    def at(self, k, t):
        """Instance k's placement at time t as float64 (3, 4): the fp32 interpolation, or M0 where that is not finite."""
        m = MM.lerp(self.t0[k], self.t1[k], t)[0]
        return (m if np.isfinite(m).all() else self.t0[k]).reshape(3, 4).astype(F64)


def _tops():
    named = E.edge_matrices()
    names = [n for n, _, _ in named]
    by_name = {n: m for n, m, _ in named}
    by_name["origin"] = E.place(np.eye(3))
    transposed = by_name["near_singular"].copy().reshape(3, 4)
    transposed[:, :3] = transposed[:, :3].T.copy()
    transposed[:, 3] = (0.0, 0.0, -32.0)                              # x = y = 0 as for NEAR_SINGULAR itself: its rows 0 and 1 then multiply zeros
    by_name["near_singular^T"] = transposed.reshape(12)
    t0, t1 = [], []
    for k, (a, b) in enumerate(EDGE_PAIRS):
        m0, m1 = by_name[a].copy(), by_name[b].copy()
        if "translation" not in a + b and "scale_2^20" not in (a, b):      # M1 takes M0's place: the pair turns and scales where it stands
            m1[3::4] = m0[3::4]
        for m, name in ((m0, a), (m1, b)):
            if name == "scale_2^20":
                m[3::4] = -(2.0 ** 20) * np.array(AIR_POINTS[k])
        t0.append(m0); t1.append(m1)
    t1[0] = t0[0] + E.place(np.zeros((3, 3)), (0.125, 0.0, -0.125))
    static = [m for _, m, _ in named]
    moved = E.COINCIDENT.copy(); moved[3::4] += F32([0.5, -0.25, 0.125])
    row0 = E.TOPS["leaf8"].transforms
    row1 = np.array([E.place(E._rot_y(0.2 * k + 0.3) * (0.6 + 0.05 * k), (3.0 * k + 0.25, 0.1 * k, 0.5 * (k % 3) - 0.25)) for k in range(8)])
    cross0, cross1 = zip(*CROSSING.values())
    return {"static_pairs": Top("static_pairs", static, static, [o for _, _, o in named], range(len(named)),
                                [names.index(n) for n in E.AXIS_ALIGNED]),
            "edge_pairs": Top("edge_pairs", t0, t1, [0] * len(t0), range(len(t0)), DIAGONAL_PAIRS),
            "crossing": Top("crossing", cross0, cross1, [0] * 4, range(4), range(4)),
            "coincident": Top("coincident", [E.COINCIDENT] * 2, [moved] * 2, [0, 0], [0], []),
            "leaf8": Top("leaf8", row0, row1, [0] * 8, range(8), [])}


TOPS = _tops()


class Scene:
    """The model's side of (top, max_leaf): the packed objects, the motion descriptors and the motion TLAS."""

    def __init__(self, block, top, max_leaf):
        self.top, self.max_leaf = top, max_leaf
        self.pairs = [block, M.flat_object()]
        self.nodes, self.tris, self.table = M.pack(self.pairs)
        self.descs = MM.descriptors(top.t0, top.t1, top.obj, top.ids)
        self.tlas, self.inst, self.info = MM.build_motion_tlas(self.nodes, self.table, self.descs, max_leaf)
        self.slot = np.zeros(int(top.ids.max()) + 1, np.int64)           # instance id -> leaf-order slot
        self.slot[self.inst["instance_id"] & 0x7FFFFFFF] = np.arange(top.n)

    def model(self):
        return self.tlas, self.inst, self.nodes, self.tris

    def object_boxes(self):
        roots = self.nodes[self.table["node_offset"][self.top.obj]]
        lo, hi = zip(*(M.object_box(r) for r in roots))
        return np.array(lo), np.array(hi)

    def num_tris_of(self, slot):
        """The triangle records of the object that the instance in leaf-order slot `slot` places (motion_instance_fixtures.brute_force)."""
        return int(self.table["num_tris"][np.flatnonzero(self.table["tri_offset"] == self.inst["tri_offset"][slot])[0]])

    def motion_boxes(self):
        return MM.motion_box(self.top.t0, self.top.t1, *self.object_boxes())


_cache = {}


def scene(block, top, max_leaf=1) -> Scene:
    key = ("scene", top, max_leaf)
    if key not in _cache:
        _cache[key] = Scene(block, TOPS[top], max_leaf)
    return _cache[key]


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------
def aimed(top, n, seed, times, targets=None):
    """n world rays, ray k aimed at instance targets[k % len] (default: top.aimed): made in object space (E._object_space; for
    NEAR_SINGULAR at a time of 0 or 1 E._dyadic_object_space), carried out through the instance's placement at the ray's own time."""
    rng = np.random.default_rng(seed)
    t = TOPS[top]
    targets = t.aimed if targets is None else targets
    org, d, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, F32)
    for j, k in enumerate(targets):
        sel = np.arange(j, n, len(targets))
        exact = any(np.array_equal(m.reshape(3, 4)[:, :3], np.asarray(E.NEAR_SINGULAR, F32)) for m in (t.t0[k], t.t1[k]))
        o, dd, tm = E._dyadic_object_space(rng, len(sel)) if exact else E._object_space(rng, len(sel), int(t.obj[k]))
        for i, r in enumerate(sel):
            m = t.at(k, times[r])
            org[r], d[r] = o[i] @ m[:, :3].T + m[:, 3], dd[i] @ m[:, :3].T
        tmax[sel] = tm
    with np.errstate(over="ignore"):
        return F.make_rays(org.astype(F32), d.astype(F32), 0.0, tmax)


def class_a(top):
    n = 4 * len(E.SPECIALS) ** 2
    times = times_for(n)
    rays = aimed(top, n, 1, times)
    k = np.arange(n)
    rays["tmin"], rays["tmax"] = E.SPECIALS[k % len(E.SPECIALS)], E.SPECIALS[(k // len(E.SPECIALS)) % len(E.SPECIALS)]
    return rays, times


def class_b(top):
    """E.class_b through the placement at the ray's time: per axis-aligned instance world axis directions +-e_a with pairs of E.BESIDE
    values on the two other axes, then rays along -e_a beside negative zeros and negative tiny values, from the air of the object."""
    t = TOPS[top]
    general = max(24, 216 // len(t.axis))
    negative = [(-0.0, -0.0), (-0.0, -1e-9), (-1e-40, -0.0), (-0.0, -1e-40)]
    n = len(t.axis) * (general + 12)
    times = times_for(n)
    org, d, tmax = [], [], []
    for j, k in enumerate(t.axis):
        inside = np.array([0.45, 0.9, 0.5]) if t.obj[k] == 0 else np.array([0.3, 0.2, 0.9])
        for r in range(general + 12):
            m = t.at(k, times[len(org)])
            if r < general:
                a, sign = (r % 6) // 2, 1.0 - 2.0 * (r % 2)
                pick = (r // 6 + 11 * (r % 6) + 5 * j) % 36
                v = [E.BESIDE[pick % 6], E.BESIDE[pick // 6]]
                tmax.append(F32(1e-9) if r % 3 == 2 else FLT_MAX)
            else:
                a, sign, v = (r - general) % 3, -1.0, list(negative[(r - general) // 3])
                tmax.append(FLT_MAX)
            d.append([sign if c == a else v.pop() for c in range(3)])
            org.append((inside + 0.01 * np.array([r % 5, r % 3, r % 7])) @ m[:, :3].T + m[:, 3])
    return F.make_rays(np.array(org).astype(F32), np.array(d, F64).astype(F32), 0.0, np.array(tmax, F32)), times


def class_c(top):
    base_times = times_for(46)
    base = aimed(top, 46, C_SEED, base_times)
    out, times = [], []
    for r, t in zip(base, base_times):
        out.append(r.copy())
        for field in ("org", "dir"):
            for c in range(3):
                for value in (np.nan, np.inf, -np.inf):
                    bad = r.copy(); bad[field][c] = value
                    out.append(bad)
        times += [t] * 19
    return np.array(out, F.RAY1), np.array(times, F32)


def class_d(block, top):
    """(rays, times, indices of the face rays): E.box_rays of the model's motion box of instance 0 (`quarter`, inside (-1, 1))."""
    rays, graze = E.box_rays(scene(block, top).motion_boxes()[0], seed=D_SEED)
    return rays, times_for(len(rays)), graze


def class_e(oracle, block, top):
    """tmax = the model's closest t, bit for bit, and the floats on either side of it, for 100 rays that hit (each at its own time)."""
    times = times_for(230)
    base = aimed(top, 230, 5, times)
    hits, _ = MM.trace(oracle, *scene(block, top).model(), base, times)
    hit = np.flatnonzero(hits["tri_id"] >= 0)[:100]
    t = hits["t"][hit]
    out = np.repeat(base[hit], 3)
    out["tmax"] = np.stack([np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))], 1).reshape(-1)
    return out, np.repeat(times[hit], 3)


def class_f(top):
    pair = [k for k, (name, _, _) in enumerate(E.edge_matrices()) if name.startswith("coincident")]
    times = times_for(184)
    return aimed(top, 184, 6, times, pair[:1] if top == "static_pairs" else None), times


def rays_of(oracle, block, top, cls):
    """(rays, times) of one class on one top."""
    key = ("rays", top, cls)
    if key not in _cache:
        _cache[key] = {"a": lambda: class_a(top), "b": lambda: class_b(top), "c": lambda: class_c(top),
                       "d": lambda: class_d(block, top)[:2], "e": lambda: class_e(oracle, block, top), "f": lambda: class_f(top)}[cls]()
    return _cache[key]


def expect(oracle, block, top, max_leaf, cls, any_hit):
    """(hits HIT1, instance ids) of the model for one ray class on one top."""
    key = ("expect", top, max_leaf, cls, any_hit, MM.lerp, MM.placed, M.invert, MM._Skipping)
    if key not in _cache:
        _cache[key] = MM.trace(oracle, *scene(block, top, max_leaf).model(), *rays_of(oracle, block, top, cls), any_hit)
    return _cache[key]


def skipped_at(top, k, times):
    """Per time whether instance k of the top is skipped."""
    t = TOPS[top]
    return np.array([M.invert(MM.lerp(t.t0[k], t.t1[k], x))[1][0] for x in np.asarray(times, F32)])


def entered(oracle, sc, rays, times, any_hit=False):
    """Per ray the object-space rays of the instances the model enters, in order: [(dir', accepted, org')]; a skipped instance leaves
    no entry."""
    rec, out = E.Recorder(oracle), []
    for k in range(len(rays)):
        rec.calls = []
        MM.trace(rec, *sc.model(), rays[k:k + 1], times[k:k + 1], any_hit)
        out.append(rec.calls)
    return out


# ---- stack layouts ----------------------------------------------------------------------------------------------------------------------
SHIFTED = E.place(np.eye(3), (0.25, 0, 0))
MIRRORED = E.place(np.diag([-1.0, 1.0, 1.0]))
STACK_TIMES = F32([0.0, 1.0, 0.25, BESIDE_HALF[0]])
# name: (object, TLAS padding levels, M1, the times cycled over the rays, whether the launch raises the flag); M0 is the identity
STACK_LAYOUTS = {name: (what, levels, SHIFTED, STACK_TIMES, flagged) for name, (what, levels, flagged) in E.STACK_LAYOUTS.items()}
# identity -> its mirror image, singular at t = 0.5 exactly: the layout of leaf_63, which overflows when its instance is entered, at a
# time that skips the instance, beside NaN and the infinities, which skip every instance
STACK_LAYOUTS["skipped_leaf_63"] = (*E.STACK_LAYOUTS["leaf_63"][:2], MIRRORED, F32([0.5, np.nan, np.inf, -np.inf]), False)
STACK_LAYOUTS["entered_leaf_63"] = (*E.STACK_LAYOUTS["leaf_63"][:2], MIRRORED, F32([0.5, BESIDE_HALF[0], np.nan, 0.25]), True)
# the same layout under the `overflow` pair turned to the z axis (the flat object's world box is then thin across the rays, which all
# cross it), at the float below 0.5: the inverse is finite in float64 and not in float32, the instance is skipped, no flag -- a kernel
# that asks isfinite of the inverse before rounding it enters the instance and raises it.  Here M1 is the pair (M0, M1).
STACK_LAYOUTS["overflow_leaf_63"] = (*E.STACK_LAYOUTS["leaf_63"][:2], (_diag(1, 1, OVERFLOW_SCALE, (0, 0, 0)), _diag(1, 1, -OVERFLOW_SCALE, (0, 0, 0))),
                                     F32([BESIDE_HALF[0]]), False)


def stack_layout(name):
    """(object pair, tlas nodes, motion instances, rays, times): E.stack_layout's with two-key records: one instance moving from the
    identity to M1 under a padded single-leaf motion TLAS; three of four rays enter the scene box, the others pass 50 units beside it."""
    what, levels, m1, cycle, _ = STACK_LAYOUTS[name]
    m0, m1 = m1 if isinstance(m1, tuple) else (E.IDENTITY, m1)
    obj = M.flat_object() if what == "flat" else chain_bvh2(40)
    nodes, tris, table = M.pack([obj])
    root, inst, info = MM.build_motion_tlas(nodes, table, MM.descriptors(m0[None], m1[None], [0], [9]), 1)
    assert info[2] == 0
    rays = E.stack_layout("leaf_62" if what == "flat" else "chain_22")[3]
    return obj, pad_bvh2_depth(root, levels), inst, rays, cycle[np.arange(len(rays)) % len(cycle)]


# ---- the named perturbations of the models ----------------------------------------------------------------------------------------------------
_LERP, _PLACED, _INVERT = MM.lerp, MM.placed, M.invert


def _st(m0, m1, t):
    m0, m1 = np.asarray(m0, F32).reshape(-1, 12), np.asarray(m1, F32).reshape(-1, 12)
    return m0, m1, np.asarray(t, F32).reshape(-1, 1)


def fused_lerp(m0, m1, t):
    """fma(t, m1, s * m0)."""
    m0, m1, t = _st(m0, m1, t)
    with np.errstate(all="ignore"):
        return M.fma32(t, m1, (F32(1) - t) * m0)


def one_product_lerp(m0, m1, t):
    """m0 + t * (m1 - m0)."""
    m0, m1, t = _st(m0, m1, t)
    with np.errstate(all="ignore"):
        return (m0 + t * (m1 - m0)).astype(F32)


def clamped_lerp(m0, m1, t):
    with np.errstate(invalid="ignore"):
        return _LERP(m0, m1, np.clip(np.asarray(t, F32), F32(0), F32(1)))


def invert32(m):
    """instance_model.invert with every operation in float32."""
    m = np.asarray(m, F32).reshape(-1, 12)
    a, b, c, tx, d, e, f, ty, g, h, i, tz = (m[:, k] for k in range(12))
    with np.errstate(all="ignore"):
        c0, c1, c2 = e * i - f * h, f * g - d * i, d * h - e * g
        det = (a * c0 + b * c1) + c * c2
        r = F32(1.0) / det
        q = [[c0 * r, (c * h - b * i) * r, (b * f - c * e) * r], [c1 * r, (a * i - c * g) * r, (c * d - a * f) * r],
             [c2 * r, (b * g - a * h) * r, (a * e - b * d) * r]]
        w = np.empty((len(m), 12), F32)
        for k in range(3):
            for j in range(3):
                w[:, 4 * k + j] = q[k][j]
            w[:, 4 * k + 3] = -((q[k][0] * tx + q[k][1] * ty) + q[k][2] * tz)
    return w, ~np.isfinite(m).all(1) | (det == 0) | ~np.isfinite(det) | ~np.isfinite(w).all(1)


def invert_checked_in_double(m):
    """instance_model.invert with isfinite(w) asked of the float64 entries, before they are rounded."""
    w, bad = _INVERT(m)
    mm = np.asarray(m, F32).reshape(-1, 12)
    huge = np.isfinite(mm).all(1) & ~np.isfinite(w).all(1)
    with np.errstate(all="ignore"):
        det = np.linalg.det(mm.reshape(-1, 3, 4)[:, :, :3].astype(F64))
    return w, bad & ~(huge & (det != 0) & np.isfinite(det))


def never_skipped(minst, t, num_nodes):
    """placed with the skip test dropped: every instance is entered with whatever inverse it has."""
    inst, skipped = _PLACED(minst, t, num_nodes)
    inst["node_offset"] = minst["node_offset"]
    return inst, np.zeros_like(skipped)


def skipped_as_at_zero(minst, t, num_nodes):
    """placed with a skipped instance still traced -- through its inverse at time 0 --: it shortens tmax, takes hits and pushes."""
    inst, skipped = _PLACED(minst, t, num_nodes)
    inst["world_to_object"][skipped] = _INVERT(minst["object_to_world0"][skipped])[0]
    inst["node_offset"] = minst["node_offset"]
    return inst, np.zeros_like(skipped)


def perturbations():
    """name: (module, attribute, replacement)."""
    return {"fused": (MM, "lerp", fused_lerp), "one_product": (MM, "lerp", one_product_lerp), "clamped": (MM, "lerp", clamped_lerp),
            "fp32_inverse": (M, "invert", invert32), "checked_in_double": (M, "invert", invert_checked_in_double),
            "never_skipped": (MM, "placed", never_skipped), "skipped_still_traced": (MM, "placed", skipped_as_at_zero)}
