"""Hand-made BVH4 / BVH8 + Tri4 hierarchies whose traversal stack is as deep as the caller asks: the wide counterpart of
conftest.chain_bvh2.  Plain module (imported the way lbvh_model.py is), used by test_wide_fixtures.py (CPU) and
test_gpu_wide_edges.py (GPU).

The stack figures below are those of the reference GPU kernel's general-arity loop (mapping_gpu.impala:136-153; oracle:
traverse_gpu_wide): entry 0 is the sentinel, a node step pops one entry and pushes every child it hits, `max_stack` of the oracle
counts the sentinel, so a ray whose stack holds P real entries at its deepest reports max_stack == P + 1.  The capacity is 64
slots: P == 63 fits, P == 64 overflows.
"""
import numpy as np

from rodent_amd import formats as F

Z0 = 200.0                     # z of triangle 0; triangle with z index g lies at Z0 + g
AWAY = 1000.0                  # x offset of a triangle that miss_every moves out of the rays' way
DIRECTION = np.float32([0.001, 0.002, 1.0])
LDS_WINDOW = {4: 16, 8: 24}    # rows of the wide kernels' LDS stack window (the KW(...) rows of the variant table in traversal.hip)


def level_fans(depth, fan, last_fan=None):
    """Leaves on each of the `depth` levels: `fan` everywhere, `last_fan` (default: fan) on the deepest."""
    return [fan] * (depth - 1) + [fan if last_fan is None else last_fan]


def chain_counts(depth, fan=1, last_fan=None, ties=False):
    """(leaves, z indices, stack peak P) of chain_wide(): every level pushes its leaves, the last level's chain slot is one more
    leaf.  With ties the second leaf of every even level that has two shares the z index of the first."""
    fans = level_fans(depth, fan, last_fan)
    dup = sum(1 for i, f in enumerate(fans) if ties and i % 2 == 0 and f >= 2)
    leaves = sum(fans) + 1
    return leaves, leaves - dup, sum(fans)


def miss_every_for(depth, fan=1, last_fan=None, ties=False):
    """The smallest k for which the DEEPEST triangle of the chain is one that misses (z index not a multiple of k)."""
    _, nz, _ = chain_counts(depth, fan, last_fan, ties)
    return next(k for k in (3, 4, 5, 7, 11) if (nz - 1) % k != 0)


def chain_wide(arity, depth, fan=1, chain_last=False, miss_every=0, ties=False, last_fan=None):
    """-> (nodes: NODE4 | NODE8, tris: TRI4).  Node i has one slot that leads to node i + 1 (box z in [1, 100], entered nearest)
    and `fan` slots (1 ... arity - 1; the deepest node: `last_fan`, so that any stack peak can be reached with a wide fan) that are
    one-packet leaves over a big triangle at z = Z0 + g, g counting up with depth; the last node's chain slot is one more leaf,
    the deepest.  Unused slots are empty (child 0, bounds +inf / -inf).  A packet holds one valid triangle: prim_id = [j, -1, -1,
    INT_MIN] (-1 ends the packet, prim_id[3] < 0 ends the leaf), n = e1 x e2.

    A ray along +z from z = 0 inside |x|, |y| < 4 hits every box: all `depth` node steps come first, each leaving its leaves on the
    stack, which therefore peaks at P = sum of the fans entries (max_stack == P + 1) before the first triangle is tested.

    chain_last=False: the chain is slot 0.  A closest-hit ray enters it first (strict <) and pops the leaves far to near, accepting
        every triangle on the way to triangle 0.  An any-hit ray pushes the chain UNDER the leaves and ends on the root's first leaf.
    chain_last=True: the chain is the slot behind the leaves.  In any-hit mode every hit child goes on top, so only this order
        makes an any-hit stack deep; in closest-hit mode the first leaf is entered "nearest so far" and then displaced by the chain,
        so the order of a level's leaves on the stack depends on the strict < between siblings.
    miss_every=k: every triangle whose z index is not a multiple of k is moved AWAY in x, its leaf box stays: an any-hit ray pops
        several entries before it finds an occluder, a closest-hit ray tests packets that reject.
    ties=True (fan >= 2): on every even level the first two leaf slots get the SAME box and coplanar duplicate triangles with
        different ids (moved away together or not at all), level 0 included -- so the nearest triangle of every hitting ray is a
        duplicated one and the id that wins is decided by sibling order and the acceptance test's <=."""
    assert arity in (4, 8) and depth >= 1 and 1 <= fan <= arity - 1 and (last_fan is None or 1 <= last_fan <= arity - 1)
    fans = level_fans(depth, fan, last_fan)
    assert not ties or fans[0] >= 2
    leaves, _, _ = chain_counts(depth, fan, last_fan, ties)
    nodes = np.zeros(depth, F.NODE4 if arity == 4 else F.NODE8)
    tris = np.zeros(leaves, F.TRI4)
    inf = np.float32(np.inf)
    nodes["bounds"][:, 0::2, :] = inf
    nodes["bounds"][:, 1::2, :] = -inf
    tris["prim_id"] = np.int32([-1, -1, -1, -2 ** 31])

    state = {"j": 0, "g": 0}

    def leaf(node, slot, same_z_as_previous=False):
        j = state["j"]
        g = state["g"] - 1 if same_z_as_previous else state["g"]
        z = np.float32(Z0 + g)
        dx = np.float32(AWAY if miss_every and g % miss_every != 0 else 0.0)
        v0, v1, v2 = np.float32([-10 + dx, -10, z]), np.float32([30 + dx, -10, z]), np.float32([-10 + dx, 30, z])
        e1, e2 = v0 - v1, v2 - v0
        t = tris[j]
        t["v0"][:, 0] = v0; t["e1"][:, 0] = e1; t["e2"][:, 0] = e2; t["n"][:, 0] = np.cross(e1, e2).astype(np.float32)
        t["prim_id"][0] = j
        node["bounds"][:, slot] = [-5, 5, -5, 5, z, z]
        node["child"][slot] = ~j
        state["j"] = j + 1
        state["g"] = g + 1

    for i in range(depth):
        node, f = nodes[i], fans[i]
        chain_slot, first_leaf = (f, 0) if chain_last else (0, 1)
        for s in range(f):
            leaf(node, first_leaf + s, same_z_as_previous=ties and i % 2 == 0 and s == 1)
        if i + 1 < depth:
            node["bounds"][:, chain_slot] = [-5, 5, -5, 5, 1, 100]
            node["child"][chain_slot] = i + 2
        else:
            leaf(node, chain_slot)
    assert state["j"] == leaves
    return nodes, tris


def chain_wide_peak(arity, peak, fan=1, **kw):
    """chain_wide() whose stack peaks at exactly `peak` entries: ceil(peak / fan) levels, the remainder on the deepest."""
    depth = -(-peak // fan)
    last = peak - (depth - 1) * fan
    return chain_wide(arity, depth, fan, last_fan=last, **kw), dict(depth=depth, fan=fan, last_fan=last)


def chain_rays(n, seed, miss_third=True, jitter=False, shuffle=False, tmax=1000.0, cut=None):
    """n rays from z = 0 along (0.001, 0.002, 1) through |x|, |y| < 4: each hits every box of a chain.  miss_third: every third
    ray starts 50 units to the side and misses the root's boxes (deep and shallow lanes in one wave).  jitter: no common
    direction; shuffle: a random order.  cut=(lo, hi): every other ray that enters the chain gets a tmax drawn from [lo, hi) --
    the leaves behind it are never pushed, so the rays of one launch differ in how deep their stacks get."""
    rng = np.random.default_rng(seed)
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2))
    if miss_third:
        org[::3, 0] += 50.0
    d = np.tile(DIRECTION, (n, 1))
    if jitter:
        d[:, :2] += rng.uniform(-1e-4, 1e-4, (n, 2)).astype("<f4")
    rays = F.make_rays(org, d, 0.0, tmax)
    if cut is not None:
        rays["tmax"][1::2] = rng.uniform(cut[0], cut[1], len(rays[1::2])).astype("<f4")
    if shuffle:
        rays = rays[rng.permutation(n)]
    return np.ascontiguousarray(rays)


def flatten_tri4(tris):
    """The valid triangles of Tri4 packets as (records with v0 / e1 / e2 of shape (3,), prim ids): what a per-triangle
    reference (test_oracle.mt_float64) reads."""
    out, ids = [], []
    for p in tris:
        for k in range(4):
            if p["prim_id"][k] == -1:
                break
            out.append((p["v0"][:, k], p["e1"][:, k], p["e2"][:, k]))
            ids.append(int(p["prim_id"][k]) & 0x7FFFFFFF)
    flat = np.zeros(len(out), np.dtype([("v0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,))]))
    for i, (v0, e1, e2) in enumerate(out):
        flat[i] = (v0, e1, e2)
    return flat, np.int32(ids)


def ray_peaks(oracle, width, nodes, tris, rays, any_hit=False):
    """Deepest stack of every ray in REAL entries (max_stack of a one-ray oracle call minus the sentinel)."""
    return np.array([oracle.traverse(width, nodes, tris, rays[i:i + 1], any_hit=any_hit, algo="gpu")[1]["max_stack"] - 1
                     for i in range(len(rays))], np.int32)
