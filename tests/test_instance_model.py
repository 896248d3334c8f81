"""tests/instance_model.py (the CPU model of instanced scenes, include/rodent_instances.h) against the oracle and against its own rules:
one identity instance is the oracle, a disjoint layout against brute force per instance, exact inverses, refusals, the TLAS's structure."""
import numpy as np
import pytest

import instance_model as M
from conftest import ambiguous_mask
from rodent_amd import formats as F

IDENTITY = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
AMBIGUOUS_CAP = 0.01                        # the cap of test_refit_model.py
LAYOUT_SEED = 5                             # chosen so that the model alone meets both conditions of the brute-force test


@pytest.fixture(scope="module")
def block(cornell):
    return cornell.blocks[2]


@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name", ["primary", "random", "edge"])
def test_one_identity_instance_is_the_oracle(oracle, cornell, block, name, any_hit):
    nodes, tris = block
    p_nodes, p_tris, table = M.pack([block])
    tlas, inst, info = M.build_tlas(p_nodes, table, M.descriptors(IDENTITY[None], [0], [7]), 1)
    assert info[2] == 0 and np.array_equal(inst["world_to_object"][0], IDENTITY)
    rays = cornell.ray_sets[name]
    ref, _ = oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)
    hits, ids = M.trace(oracle, tlas, inst, p_nodes, p_tris, rays, any_hit)
    assert hits.tobytes() == ref.tobytes()
    assert np.array_equal(ids, np.where(ref["tri_id"] >= 0, 7, -1))


def disjoint_layout(seed):
    """9 rotated, scaled (some mirrored) Cornell boxes on a grid whose cells are wider than any of them, and segments across it."""
    rng = np.random.default_rng(seed)
    t = M.seeded_transforms(9, seed, 0.0, 1)[0].reshape(9, 3, 4)
    t[:, :, :3] *= np.float32(0.75)                                   # scales 0.375 ... 1.5 of a box of radius < 1.8: under 2.7
    gx, gz = np.meshgrid(np.arange(3), np.arange(3))
    t[:, 0, 3], t[:, 1, 3], t[:, 2, 3] = 8 * gx.reshape(-1), 0, 8 * gz.reshape(-1)
    lo, hi = np.float32([-4, -3, -4]), np.float32([20, 4, 20])
    a, b = rng.uniform(lo, hi, (4096, 3)).astype(np.float32), rng.uniform(lo, hi, (4096, 3)).astype(np.float32)
    return t.reshape(9, 12), F.make_rays(a, b - a, 0.0, 1.0)


def test_disjoint_layout_against_brute_force(oracle, block):
    nodes, tris = block
    p_nodes, p_tris, table = M.pack([block])
    transforms, rays = disjoint_layout(LAYOUT_SEED)
    tlas, inst, info = M.build_tlas(p_nodes, table, M.descriptors(transforms, np.zeros(9, np.int32)), 1)
    assert info[2] == 0
    # the world boxes are pairwise disjoint
    leaves = M.world_box(transforms, *(np.repeat(x[None], 9, 0) for x in M.object_box(p_nodes[0])))
    for i in range(9):
        for j in range(i):
            assert (leaves[i, 0::2] > leaves[j, 1::2]).any() or (leaves[j, 0::2] > leaves[i, 1::2]).any()
    hits, ids = M.trace(oracle, tlas, inst, p_nodes, p_tris, rays)
    # brute force per instance on the transformed rays, the minimum over the instances
    o_org, o_dir = M._object_rays(inst, rays)
    per, seconds = [], []
    for j in range(9):
        local = rays.copy(); local["org"], local["dir"] = o_org[:, j], o_dir[:, j]
        h, s = oracle.brute_force(tris, local)
        per.append(h); seconds.append(s)
    per, seconds = np.array(per), np.array(seconds)                                  # instance, ray
    t = np.where(per["tri_id"] >= 0, per["t"], np.inf)
    win = np.argmin(t, 0)
    r = np.arange(len(rays))
    best, best_inst = per[win, r], inst["instance_id"][win] & 0x7FFFFFFF
    others = t.copy(); others[win, r] = np.inf
    second = np.fmin(others.min(0), seconds[win, r]).astype(np.float32)              # the next distance in any instance
    bhit, mhit = best["tri_id"] >= 0, hits["tri_id"] >= 0
    best_inst = np.where(bhit, best_inst, -1)
    amb = ambiguous_mask(best, second)
    print(f"hit share {bhit.mean():.4f}, ambiguous share {amb.mean():.4f}")
    assert 0.1 < bhit.mean() < 0.98 and amb.mean() <= AMBIGUOUS_CAP
    assert not (bhit & ~mhit).any(), "the model misses a ray that brute force hits"
    assert np.array_equal(mhit, bhit)
    assert np.array_equal(hits["t"][bhit].view("<u4"), best["t"][bhit].view("<u4"))
    differ = bhit & ((hits["tri_id"] != best["tri_id"]) | (ids != best_inst))
    assert not (differ & ~amb).any()


def test_exact_inverses():
    rng = np.random.default_rng(3)
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    m = np.zeros((48, 3, 4), np.float32)
    for k in range(48):
        p = perms[k % 6]
        for row in range(3):
            m[k, row, p[row]] = np.float32((-1) ** (k >> (row + 1) & 1) * 2.0 ** rng.integers(-6, 7))
        m[k, :, 3] = rng.integers(-1000, 1000, 3)
    w, bad = M.invert(m.reshape(48, 12))
    assert not bad.any()
    full = lambda a: np.concatenate([a.reshape(-1, 3, 4).astype(np.float64), np.tile([[[0, 0, 0, 1.0]]], (len(a), 1, 1))], 1)
    assert np.array_equal(full(w) @ full(m), np.tile(np.eye(4), (48, 1, 1)))
    assert np.array_equal(full(m) @ full(w), np.tile(np.eye(4), (48, 1, 1)))


def test_refusals(block):
    p_nodes, _, table = M.pack([block, block])
    good = np.tile(IDENTITY, (4, 1))
    build = lambda t, obj: M.build_tlas(p_nodes, table, M.descriptors(t, obj), 2)[2][2]
    assert build(good, [0, 1, 1, 0]) == 0
    singular = good.copy(); singular[2, 8:11] = singular[2, 0:3]                 # row 2 = row 0
    assert build(singular, [0, 1, 1, 0]) == M.BAD_TRANSFORM
    nan = good.copy(); nan[1, 7] = np.nan
    assert build(nan, [0, 1, 1, 0]) == M.BAD_TRANSFORM
    inf = good.copy(); inf[3, 0] = np.inf
    assert build(inf, [0, 1, 1, 0]) == M.BAD_TRANSFORM
    tiny = good.copy(); tiny[0, 0], tiny[0, 3] = np.float32(1e-20), np.float32(1e30)   # the inverse's translation overflows fp32
    assert build(tiny, [0, 1, 1, 0]) == M.BAD_TRANSFORM
    assert build(good, [0, 2, 1, 0]) == M.BAD_OBJECT and build(good, [0, 1, -1, 0]) == M.BAD_OBJECT
    assert build(nan, [5, 1, 1, 0]) == M.BAD_OBJECT | M.BAD_TRANSFORM


def check_structure(tlas, inst, info, n, max_leaf):
    """Every instance in exactly one leaf, a sentinel at the end of every leaf, every child box around the boxes below it.  Returns
    every instance's world box as the leaves hold it."""
    assert info[0] == len(tlas) and len(inst) == n
    seen = np.zeros(n, int)
    last = inst["instance_id"] < 0

    def box_of(i, k):
        b = tlas[i]["bounds"][6 * k: 6 * k + 6]
        c = tlas[i]["child"][k]
        if c > 0:
            below = [box_of(c - 1, s) for s in (0, 1) if tlas[c - 1]["child"][s] != 0]
            lo, hi = np.min([x[0::2] for x in below], 0), np.max([x[1::2] for x in below], 0)
            assert (b[0::2] <= lo).all() and (b[1::2] >= hi).all()
        elif c < 0:
            first = ~c
            end = first + int(np.argmax(last[first:]))
            assert last[end] and not last[first:end].any() and end - first + 1 <= max_leaf
            seen[first:end + 1] += 1
        return b
    depth = lambda i: 1 + max([depth(c - 1) for c in tlas[i]["child"] if c > 0], default=0)
    for k in (0, 1):
        if tlas[0]["child"][k] != 0:
            box_of(0, k)
    assert (seen == 1).all() and info[1] == depth(0)


@pytest.mark.parametrize("max_leaf", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 65, 1000])
def test_structure(block, n, max_leaf):
    flat = M.flat_object()
    p_nodes, p_tris, table = M.pack([block, flat])
    transforms, obj = M.seeded_transforms(n, n + max_leaf, 40.0, 2)
    ids = np.arange(n) * 3 + 1
    tlas, inst, info = M.build_tlas(p_nodes, table, M.descriptors(transforms, obj, ids), max_leaf)
    assert info[2] == 0
    if n <= max_leaf:                                                    # the single-leaf root: the other slot empty
        assert info[0] == 1 and list(tlas[0]["child"]) == [~0, 0] and np.isinf(tlas[0]["bounds"][6:]).all()
    check_structure(tlas, inst, info, n, max_leaf)
    assert sorted(inst["instance_id"] & 0x7FFFFFFF) == sorted(ids)
    # a leaf's box is the union of its instances' widened world boxes, each of which contains the exact image of its object's corners
    w, bad = M.invert(transforms)
    assert not bad.any()
    order = np.argsort(ids)[np.searchsorted(np.sort(ids), inst["instance_id"] & 0x7FFFFFFF)]
    assert np.array_equal(inst["world_to_object"], w[order]) and np.array_equal(inst["node_offset"], table["node_offset"][obj[order]])
    boxes = M.world_box(transforms, *np.array([M.object_box(p_nodes[o]) for o in table["node_offset"][obj]]).transpose(1, 0, 2))
    m64 = transforms.reshape(n, 3, 4).astype(np.float64)
    for k in range(n):
        lo, hi = (x.astype(np.float64) for x in M.object_box(p_nodes[table["node_offset"][obj[k]]]))
        corners = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)])
        image = corners @ m64[k, :, :3].T + m64[k, :, 3]
        assert (boxes[k, 0::2] <= image.min(0)).all() and (boxes[k, 1::2] >= image.max(0)).all()
