"""The chunk loops' step of the default BVH2 kernel (k_bvh2_top_auto; bvh2_step / trace_chunk, DESIGN 3.1, LAB_NOTES 18): the chunk loop
runs per lane (`while (top != 0)`), and the two rare stack events -- a window that fills, a block that comes back -- share one
wave-uniform cold block.  (A third form, one lane mask that chooses the child a lane goes on with, was built and measured with them and
is not shipped; its cases stay: they hold for any statement of the child selection.)

None of it may change what a lane loads, tests or stores: whichever loop and whichever record form runs, every Hit1 record is the CPU
oracle's, byte for byte, closest and any hit.  The cases are the ones in which the forms could differ from the statements they
replace: every class of lane at one node in one wave iteration, lanes that finish first and last, and a spill beside a reload.

Small launches reach the kernel through rodent_hip_top_min_rays(0) and variant "top", as in test_gpu_record_offsets.py.
"""
import numpy as np
import pytest

from rodent_amd import formats as F

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
WINDOW, SPILL_ROWS = 15, 7          # the lanes' LDS window (rows), the entries that move out together (kSpillRows, traversal_device.h)


@pytest.fixture(scope="module")
def gpu(native_build):
    import torch
    from rodent_amd import abi
    assert torch.cuda.is_available(), "these tests need a GPU"
    abi.top_min_rays(0)                 # every default launch through k_bvh2_top_auto
    yield abi
    abi.top_min_rays(-1)
    abi.record_offsets(True)
    abi.octant_loops(True)


def run_all_forms(gpu, oracle, bvh, nodes, tris, rays, what, octants=None, refs=None):
    """Octant loops on and off, offset and 64-bit records, closest and any hit: the oracle's records.  octants: (lowest, highest) stats[3]
    of a launch with the octant loops on (workgroup 0's chunks that took one)."""
    top = gpu.variants(2).index("top")
    if refs is None:
        refs = {any_hit: oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)[0] for any_hit in (False, True)}
    try:
        for loops in (True, False):
            gpu.octant_loops(loops)
            for offsets in (True, False):
                gpu.record_offsets(offsets)
                for any_hit in (False, True):
                    gpu.read_stats(0)
                    got = gpu.traverse(bvh, rays, any_hit=any_hit, variant=top)
                    st = gpu.read_stats(0)
                    ref = refs[any_hit]
                    bad = np.nonzero((got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4)).any(axis=1))[0]
                    assert got.tobytes() == ref.tobytes(), (what, loops, offsets, any_hit, bad[:4], got[bad[:2]], ref[bad[:2]])
                    # (DeviceBvh keeps both arrays in one allocation: the offset form whenever the switch is on)
                    assert (int(st[1]), int(st[0])) == ((1, 0) if offsets else (0, 1)), (what, loops, offsets, any_hit, st)
                    if octants is not None:
                        lo, hi = octants if loops else (0, 0)
                        assert lo <= int(st[3]) <= hi, (what, loops, offsets, any_hit, st)
    finally:
        gpu.octant_loops(True)
        gpu.record_offsets(True)
    return refs


# ---- child selection ---------------------------------------------------------------------------------------------------------------------

WORLD = (-100.0, 100.0)


def slab_box(axis, lo, hi):
    b = [WORLD[0], WORLD[1]] * 3
    b[2 * axis], b[2 * axis + 1] = lo, hi
    return b


def plane_triangle(axis, c):
    """A triangle in the plane `axis` = c that covers the world box there."""
    p = np.full((3, 3), -1000.0, np.float32)
    p[:, axis] = c
    p[1, (axis + 1) % 3] = 3000.0
    p[2, (axis + 2) % 3] = 3000.0
    return p


def slab_tree():
    """24 inner nodes, every number exact in float32 for rays along (1, 1, 1):
      node 1        child 0: the slab 10 <= x <= 20 (node 2), child 1: the slab 10 <= y <= 20 (node 3)
      node 2        two children with the SAME box (the x slab): nodes 4 and 5 -- a tie whatever the ray
      node 3        child 0: the y slab (node 6), child 1: an empty slot (id 0, box +inf / -inf)
      nodes 4, 5, 6 the slab halved three times (seven nodes each), the halves in near-far order on even levels and far-near on odd ones;
                    every leaf holds one triangle, a plane across the middle of its eighth of the slab."""
    nodes, tris = [], []

    def new_node():
        nodes.append(None)
        return len(nodes)                                      # 1-based id

    def put(node_id, box0, box1, c0, c1):
        rec = np.zeros((), F.NODE2)
        rec["bounds"] = list(box0) + list(box1)
        rec["child"] = [c0, c1]
        nodes[node_id - 1] = rec

    def leaf(axis, lo, hi):
        p = plane_triangle(axis, (lo + hi) / 2)
        t = np.zeros((), F.TRI1)
        t["v0"] = p[0]; t["e1"] = p[0] - p[1]; t["e2"] = p[2] - p[0]
        t["prim_id"] = np.int32(len(tris)) | np.int32(-2 ** 31)
        tris.append(t)
        return ~(len(tris) - 1)

    def subtree(node_id, axis, lo, hi, level):
        mid = (lo + hi) / 2
        halves = [(lo, mid), (mid, hi)] if level % 2 == 0 else [(mid, hi), (lo, mid)]
        if level == 2:
            kids = [leaf(axis, a, b) for a, b in halves]
        else:
            kids = [new_node(), new_node()]
            for k, (a, b) in zip(kids, halves):
                subtree(k, axis, a, b, level + 1)
        put(node_id, slab_box(axis, *halves[0]), slab_box(axis, *halves[1]), kids[0], kids[1])

    root, nx, ny = new_node(), new_node(), new_node()
    put(root, slab_box(0, 10, 20), slab_box(1, 10, 20), nx, ny)
    a, b = new_node(), new_node()
    put(nx, slab_box(0, 10, 20), slab_box(0, 10, 20), a, b)
    c = new_node()
    put(ny, slab_box(1, 10, 20), [INF, -INF] * 3, c, 0)
    subtree(a, 0, 10.0, 20.0, 0)
    subtree(b, 0, 10.0, 20.0, 0)
    subtree(c, 1, 10.0, 20.0, 0)
    return np.array(nodes, F.NODE2), np.array(tris, F.TRI1)


def slab_interval(lo, hi, o):
    """[entry, exit] of a ray from coordinate o along +1 through lo <= coordinate <= hi, and whether it is hit from tmin = 0."""
    te, tx = np.float32(lo) - np.float32(o), np.float32(hi) - np.float32(o)
    return te, tx, max(te, np.float32(0)) <= tx


def test_every_lane_class_at_one_node_in_one_iteration(gpu, oracle):
    nodes, tris = slab_tree()
    assert len(nodes) == 24 and len(tris) == 24
    # one 8 x 8 tile of parallel rays along (1, 1, 1): lane (i, j) starts at x = xs[i], y = xs[j]; the root's slabs are x and y
    xs = np.float32([0.0, 3.0, 5.0, 8.5, 12.0, 19.0, 30.0, 45.0])
    org = np.zeros((64, 3), np.float32)
    org[:, 0], org[:, 1] = np.repeat(xs, 8), np.tile(xs, 8)
    rays = F.make_rays(org, np.ones((64, 3), np.float32), 0.0, 1000.0)
    # the classes at the root, which every lane tests in the chunk's FIRST wave iteration
    classes = set()
    for o in org:
        te0, _, h0 = slab_interval(10, 20, o[0])
        te1, _, h1 = slab_interval(10, 20, o[1])
        te0, te1 = max(te0, np.float32(0)), max(te1, np.float32(0))
        classes.add(("only 0" if h0 else "neither") if not h1 else "only 1" if not h0 else
            "0 nearer" if te0 < te1 else "1 nearer" if te0 > te1 else "tie")
    assert classes == {"only 0", "only 1", "0 nearer", "1 nearer", "tie", "neither"}, classes
    ref = oracle.traverse(2, nodes, tris, rays)[0]
    steps = oracle.ray_steps(nodes, tris, rays)
    assert steps[:, 0].min() == 1 and steps[:, 0].max() > 12        # the lanes that miss both slabs; the ones that cross both
    assert (ref["tri_id"] < 0).sum() == 4 and len(set(ref["tri_id"])) >= 6
    # node 2's identical boxes: the strict `<` sends every ray into child 1 (node 5) first and node 4 is traced behind it, where the same
    # triangle at the same t replaces the record -- a ray through the x slab alone ends in node 4's copy (ids 0 .. 7), not node 5's (8 .. 15)
    x_only = (org[:, 0] < 20) & (org[:, 1] > 20)
    assert x_only.any() and ((ref["tri_id"][x_only] >= 0) & (ref["tri_id"][x_only] < 8)).all(), ref["tri_id"][x_only]
    bvh = gpu.DeviceBvh(2, nodes, tris, 0)
    run_all_forms(gpu, oracle, bvh, nodes, tris, rays, "slab tree", octants=(1, 1))
    # the same tile seen from the other side (octant 7): mirrored origins, direction (-1, -1, -1) -- the mirrored tree
    mirrored = nodes.copy()
    b = nodes["bounds"].reshape(-1, 2, 3, 2)
    mirrored["bounds"] = np.stack([-b[..., 1], -b[..., 0]], -1).reshape(-1, 12)
    mtris = tris.copy()
    for k in ("v0", "e1", "e2"):
        mtris[k] = -tris[k]
    mrays = F.make_rays(np.float32(0.0) - org, -np.ones((64, 3), np.float32), 0.0, 1000.0)
    mref = oracle.traverse(2, mirrored, mtris, mrays)[0]
    assert np.array_equal(mref["tri_id"], ref["tri_id"])
    run_all_forms(gpu, oracle, gpu.DeviceBvh(2, mirrored, mtris, 0), mirrored, mtris, mrays, "slab tree, octant 7", octants=(1, 1))


# ---- loop form -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell_dev(gpu, cornell):
    return gpu.DeviceBvh(2, *cornell.blocks[2], 0)


def test_a_padded_last_chunk(gpu, oracle, cornell, cornell_dev):
    from test_gpu_octant_loops import CORNELL_EYE, octant_dirs
    nodes, tris = cornell.blocks[2]
    n = 64 + 37
    rays = F.make_rays(np.tile(CORNELL_EYE, (n, 1)), octant_dirs(np.random.default_rng(37), 6, n), 0.0, 100.0)
    run_all_forms(gpu, oracle, cornell_dev, nodes, tris, rays, "64 + 37 rays", octants=(1, 2))


def test_first_lane_ends_at_once_and_last_lane_is_the_longest(gpu, oracle, cornell, cornell_dev):
    """Parallel rays into the Cornell box: lane 0 passes beside it and is done after the root, lane 63 holds the ray with the most steps of
    the chunk (and the lanes between them end one after the other)."""
    nodes, tris = cornell.blocks[2]
    b = nodes[0]["bounds"]
    lo = np.float32([min(b[0], b[6]), min(b[2], b[8]), min(b[4], b[10])]); hi = np.float32([max(b[1], b[7]), max(b[3], b[9]), max(b[5], b[11])])
    rng = np.random.default_rng(63)
    d = np.float32([0.05, -0.07, -1.0])
    org = rng.uniform(lo, hi, (256, 3)).astype(np.float32)
    org[:, 2] = hi[2] + np.float32(1.0)
    pool = F.make_rays(org, np.tile(d, (256, 1)), 0.0, 100.0)
    steps = oracle.ray_steps(nodes, tris, pool).astype(np.int64).sum(axis=1)
    order = np.argsort(steps, kind="stable")[np.linspace(0, 255, 63).astype(int)]   # 63 rays by rising length: the longest one last
    rays = pool[np.concatenate([[0], order])].copy()
    rays["org"][0] = [hi[0] + 50.0, hi[1] + 50.0, hi[2] + 1.0]                 # lane 0: beside the box
    steps = oracle.ray_steps(nodes, tris, rays).astype(np.int64)
    assert tuple(steps[0]) == (1, 0), steps[0]
    total = steps.sum(axis=1)
    assert total[63] == total.max() and total[63] > 8 * total[0] and len(set(total)) >= 5, total
    run_all_forms(gpu, oracle, cornell_dev, nodes, tris, rays, "lane 0 ends first, lane 63 last", octants=(1, 1))
    # ... and a chunk whose rays ALL pass beside the box: the loop ends after one iteration
    rays["org"][:, 0] += np.float32(500.0)
    refs = run_all_forms(gpu, oracle, cornell_dev, nodes, tris, rays, "every ray misses", octants=(1, 1))
    assert (refs[False]["tri_id"] == -1).all() and (oracle.ray_steps(nodes, tris, rays) == (1, 0)).all()


def test_two_chunks_of_different_octants_in_one_wave(gpu, oracle, cornell, cornell_dev):
    """A launch with more chunks than resident waves: the chunks behind the waves' first ones are drawn by waves that have traced a chunk
    already.  Every first chunk is of one of the octants 0 .. 6 and every later one of octant 7, so a wave that draws again leaves one
    octant's loop and enters another's."""
    import torch
    from test_gpu_octant_loops import CORNELL_EYE, SIGNS
    nodes, tris = cornell.blocks[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = ((cus * 2 + 63) // 64) * 64                    # persistent_groups(32 waves per CU, 16 per workgroup)
    stripe_tickets = (groups // 64) * 16 * 64               # a stripe's first draws (stripe_rank / ray_of, traversal_top.h)
    first = groups * 16                                     # chunks
    # the smallest launch that holds every first draw and 64 chunks + 37 rays behind them
    later = 64
    c = 0
    while True:
        t = ((c // 32) // 64) * 2048 + (c % 32) * 64
        later -= t >= stripe_tickets
        c += 1
        if later == 0:
            break
    n = c * 64 + 37
    chunk = np.arange(n) // 64
    ticket = ((chunk // 32) // 64) * 2048 + (chunk % 32) * 64
    is_later = ticket >= stripe_tickets
    assert (~is_later[::64]).sum() == first and is_later[::64].sum() == 65
    octant = np.where(is_later, 7, chunk % 7)
    rng = np.random.default_rng(77)
    d = rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32) * np.stack(SIGNS)[octant]
    rays = F.make_rays(np.tile(CORNELL_EYE, (n, 1)), d.astype(np.float32), 0.0, 100.0)
    # workgroup 0: its sixteen first chunks, and whatever it draws of the 65 later ones
    run_all_forms(gpu, oracle, cornell_dev, nodes, tris, rays, f"{n} rays", octants=(16, 16 + 65))


# ---- spill and reload --------------------------------------------------------------------------------------------------------------------

def two_chains(depth_a, lead_a, depth_b):
    """conftest.chain_bvh2 twice under one root: chain A (x < 0) behind `lead_a` nodes with one child and one empty slot, chain B (x > 0)
    right under the root.  Returns nodes, tris."""
    from conftest import chain_bvh2
    na, ta = chain_bvh2(depth_a)
    nb, tb = chain_bvh2(depth_b)
    head = np.zeros(1 + lead_a, F.NODE2)
    first_a, first_b = 1 + lead_a + 1, 1 + lead_a + depth_a + 1             # 1-based ids of the chains' first nodes
    box_a, box_b, empty = [-5, -1, -5, 5, 1, 1000], [1, 5, -5, 5, 1, 1000], [INF, -INF] * 3
    head[0]["bounds"] = box_a + box_b
    head[0]["child"] = [2 if lead_a else first_a, first_b]
    for i in range(lead_a):
        head[1 + i]["bounds"] = box_a + empty
        head[1 + i]["child"] = [3 + i if i + 1 < lead_a else first_a, 0]
    for chain, tri_chain, first_node, first_tri, (x0, x1) in ((na, ta, first_a, 0, (-5, -1)), (nb, tb, first_b, len(ta), (1, 5))):
        child = chain["child"]
        inner = child > 0
        child[inner] += first_node - 1
        child[~inner] = ~(~child[~inner] + first_tri)
        chain["bounds"][:, [0, 6]] = x0
        chain["bounds"][:, [1, 7]] = x1
        tri_chain["prim_id"] = (np.arange(len(tri_chain), dtype=np.int32) + np.int32(first_tri)) | np.int32(-2 ** 31)
    return np.concatenate([head, na, nb]), np.concatenate([ta, tb])


def chain_events(depth, lead):
    """Wave iterations (1-based; the root's step is iteration 1) in which a ray down a chain_bvh2(depth) behind `lead` one-child nodes
    spills a block and reloads one.  Push p happens in iteration 1 + lead + p; the push that fills row WINDOW moves SPILL_ROWS entries out;
    after the last node every iteration tests one triangle and pops one entry, and the pop of row 0 brings a block back."""
    spills, window = [], 0
    for p in range(1, depth + 1):
        window += 1
        if window == WINDOW:
            spills.append(1 + lead + p)
            window -= SPILL_ROWS
    reloads, it = [], 1 + lead + depth
    for _ in spills:
        it += window + 1                                   # the entries in the window, then row 0
        reloads.append(it)
        window = SPILL_ROWS - 1                             # the block's newest entry is the new top
    return spills, reloads, it + window + 1                # ... and the iteration that pops the final 0


def test_a_spill_beside_a_reload_in_one_iteration(gpu, oracle):
    """Depths 16 (one block moves out) and 63 (all seven) in one wave: the short chain's ray reloads its block in the very iteration in
    which the long chain's ray spills its third."""
    depth_a, lead_a, depth_b = 16, 3, 63
    spills_a, reloads_a, end_a = chain_events(depth_a, lead_a)
    spills_b, reloads_b, end_b = chain_events(depth_b, 0)
    assert len(spills_a) == 1 and len(spills_b) == 7
    assert reloads_a[0] == spills_b[2] == 30, (reloads_a, spills_b)
    nodes, tris = two_chains(depth_a, lead_a, depth_b)
    rng = np.random.default_rng(16)
    n = 64
    org = np.zeros((n, 3), np.float32)
    org[:, 0] = np.where(np.arange(n) % 2 == 0, -3.0, 3.0) + rng.uniform(-1, 1, n)   # even lanes chain A, odd lanes chain B
    org[:, 1] = rng.uniform(-4, 4, n)
    org[5::16, 0] += np.float32(50.0)                                                # a few lanes beside both
    rays = F.make_rays(org, np.tile(np.float32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 2000.0)
    # the oracle's step counts say that the rays walk the chains as the model assumes: (nodes, triangles) per ray, and the iteration count
    steps = oracle.ray_steps(nodes, tris, rays).astype(np.int64)
    depths = oracle.ray_depths(nodes, tris, rays)
    a, b = np.arange(n) % 2 == 0, np.arange(n) % 2 == 1
    beside = org[:, 0] > 40
    assert (steps[a & ~beside] == (1 + lead_a + depth_a, depth_a + 1)).all() and (depths[a & ~beside] == depth_a).all()
    assert (steps[b & ~beside] == (1 + depth_b, depth_b + 1)).all() and (depths[b & ~beside] == depth_b).all()
    assert steps[a & ~beside].sum(axis=1)[0] == end_a and steps[b & ~beside].sum(axis=1)[0] == end_b
    assert (steps[beside] == (1, 0)).all() and beside.sum() == 4
    bvh = gpu.DeviceBvh(2, nodes, tris, 0)
    refs = run_all_forms(gpu, oracle, bvh, nodes, tris, rays, "two chains", octants=(1, 1))
    assert set(refs[False]["tri_id"]) == {-1, 0, depth_a + 1}
    # stats[7]: one block per spill and lane
    gpu.read_stats(0)
    gpu.traverse(bvh, rays, variant=gpu.variants(2).index("top"))
    assert int(gpu.read_stats(0)[7]) == int((a & ~beside).sum()) * 1 + int((b & ~beside).sum()) * 7


def test_a_ray_deeper_than_the_stack_raises_the_flag(gpu, oracle):
    """64 entries: the seven blocks are out and the window fills again.  The launch reports the overflow (once: the report clears it), in
    either loop and either record form, beside rays that spill and reload; launches that stay within 63 entries are unaffected afterwards."""
    nodes, tris = two_chains(16, 3, 64)
    n = 64
    org = np.zeros((n, 3), np.float32)
    org[:, 0] = -3.0
    org[63, 0] = 3.0                                                                 # the one ray down the 64-deep chain
    rays = F.make_rays(org, np.tile(np.float32([0.001, 0.002, 1.0]), (n, 1)), 0.0, 2000.0)
    assert oracle.ray_depths(nodes, tris, rays[:63]).max() == 16
    with pytest.raises(RuntimeError, match="stack overflow"):                         # the oracle's 64 slots hold 63 entries and a sentinel
        oracle.traverse(2, nodes, tris, rays[63:])
    bvh = gpu.DeviceBvh(2, nodes, tris, 0)
    top = gpu.variants(2).index("top")
    try:
        for loops in (True, False):
            gpu.octant_loops(loops)
            for offsets in (True, False):
                gpu.record_offsets(offsets)
                for any_hit in (False, True):
                    with pytest.raises(RuntimeError, match="stack overflow"):
                        gpu.traverse(bvh, rays, any_hit=any_hit, variant=top)
                    assert gpu.lib().rodent_hip_check_errors(0, None) == 0           # cleared by the report
    finally:
        gpu.octant_loops(True)
        gpu.record_offsets(True)
    run_all_forms(gpu, oracle, bvh, nodes, tris, rays[:63], "the 63 rays of the 16-deep chain", octants=(1, 1))
