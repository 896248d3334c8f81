"""Record offsets of the default BVH2 kernel (k_bvh2_top_auto<.., OFFS>; rodent_hip_record_offsets).

Where the node and the triangle array lie less than 4 GiB apart and neither mapped range could hold 2^23 records, a lane addresses its
record as ONE scalar base (the lower of the two pointers) + a 32-bit byte offset; any other launch, and every launch with the switch off,
builds 64-bit addresses from two 64-bit bases as before.  The addresses are the same addresses: whichever form runs, every Hit1 record is
the CPU oracle's, byte for byte.  stats[1] / stats[0] count the launches that took the offset / the 64-bit form.

Small launches reach the kernel through rodent_hip_top_min_rays(0) and variant "top", as in test_gpu_octant_loops.py.
"""
import numpy as np
import pytest

from rodent_amd import formats as F

GiB = 1 << 30
MAX_IDS = (1 << 23) - 1             # v_mad_i32_i24: |top| < 2^23 (kOffsetIdBits, traversal.hip)


# ---- the predicate: no GPU --------------------------------------------------------------------------------------------------------------

def test_predicate_on_made_up_pointers(native_build):
    from rodent_amd import abi
    ok = abi.record_offsets_ok
    a = 0x7F00_0000_0000
    mb = 1 << 20
    # (nodes, node bytes, tris, tri bytes) -> expected
    cases = [
        # two small arrays next to each other, either order
        ((a, mb, a + mb, mb), True),
        ((a + mb, mb, a, mb), True),
        # from the lower pointer to the end of the farther range: one byte under 4 GiB, exactly 4 GiB, one byte over -- nodes lower
        ((a, mb, a + 4 * GiB - mb - 1, mb), True),
        ((a, mb, a + 4 * GiB - mb, mb), False),
        ((a, mb, a + 4 * GiB - mb + 1, mb), False),
        # ... and triangles lower
        ((a + 4 * GiB - mb - 1, mb, a, mb), True),
        ((a + 4 * GiB - mb, mb, a, mb), False),
        ((a + 4 * GiB - mb + 1, mb, a, mb), False),
        # the pointers themselves less than 4 GiB apart, the farther range's END beyond: a lane could address a byte out of reach
        ((a, mb, a + 4 * GiB - 16, mb), False),
        ((a + 4 * GiB - 16, mb, a, mb), False),
        # far apart
        ((a, mb, a + 64 * GiB, mb), False),
        ((a + 64 * GiB, mb, a, mb), False),
        # the lower range is the long one and reaches past the other
        ((a, 2 * GiB, a + mb, mb), False),                        # 2 GiB of nodes: 2^25 ids
        ((a, 64 * MAX_IDS, a + mb, mb), True),
        # ids on either side of the multiply's operand limit: 2^23 - 1 records fit, 2^23 do not (63 / 47 spare bytes hold no record)
        ((a, 64 * MAX_IDS, a + GiB, 48 * MAX_IDS), True),
        ((a, 64 * MAX_IDS + 63, a + GiB, 48 * MAX_IDS + 47), True),
        ((a, 64 * (MAX_IDS + 1), a + GiB, mb), False),
        ((a, mb, a + GiB, 48 * (MAX_IDS + 1)), False),
        ((a + GiB, 64 * (MAX_IDS + 1), a, mb), False),
        ((a + GiB, mb, a, 48 * (MAX_IDS + 1)), False),
        # zero-length arrays: the runtime does not know the pointer, nothing bounds its ids
        ((a, 0, a + mb, mb), False),
        ((a, mb, a + mb, 0), False),
        ((a, 0, a, 0), False),
        ((0, 0, 0, 0), False),
        # one record each, touching
        ((a, 64, a + 64, 48), True),
        ((a + 48, 64, a, 48), True),
        # a range that would wrap the address space is no range
        (((1 << 64) - mb, 2 * mb, (1 << 64) - 8 * mb, mb), False),
    ]
    for args, expected in cases:
        assert ok(*args) is expected, ([hex(x) for x in args], expected)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------

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


def carve(gpu, nodes, tris, nodes_first, distance, tail=0):
    """nodes and tris in ONE device buffer: the lower array at byte 0 (behind a 256-byte guard), the other `distance` bytes above its
    start (at least the lower array's size, 16-byte aligned); `tail`: bytes of the buffer behind the upper array.  The guard and every
    gap hold 0xFF bytes (NaN bounds, ids that are no ids)."""
    import torch
    nb, tb = nodes.view(np.uint8).reshape(-1), tris.view(np.uint8).reshape(-1)
    lower, upper = (nb, tb) if nodes_first else (tb, nb)
    guard = 256
    start = guard + max(distance, (len(lower) + 15) // 16 * 16)
    assert start % 16 == 0
    host = np.full(start + len(upper) + tail, 0xFF, np.uint8)
    host[guard:guard + len(lower)] = lower
    host[start:start + len(upper)] = upper
    buf = torch.from_numpy(host).to("cuda:0")
    lo_t, up_t = buf[guard:guard + len(lower)], buf[start:start + len(upper)]
    node_t, tri_t = (lo_t, up_t) if nodes_first else (up_t, lo_t)
    bvh = gpu.DeviceBvh.from_tensors(2, node_t, tri_t, len(nodes), len(tris), 0)
    bvh.keep = buf
    return bvh, start - guard


def run_both_forms(gpu, oracle, bvh, nodes, tris, rays, what, expect_offsets=True, octants=None, refs=None):
    """Closest and any hit, switch on and off: the oracle's records, and the stats word names the form that ran."""
    top = gpu.variants(2).index("top")
    if refs is None:
        refs = {any_hit: oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)[0] for any_hit in (False, True)}
    try:
        for on in (True, False):
            gpu.record_offsets(on)
            for any_hit in (False, True):
                gpu.read_stats(0)
                got = gpu.traverse(bvh, rays, any_hit=any_hit, variant=top)
                st = gpu.read_stats(0)
                ref = refs[any_hit]
                bad = np.nonzero((got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4)).any(axis=1))[0]
                assert got.tobytes() == ref.tobytes(), (what, on, any_hit, bad[:4], got[bad[:2]], ref[bad[:2]])
                if on and expect_offsets is None:                  # two allocations, wherever the allocator put them
                    assert (int(st[1]), int(st[0])) in ((1, 0), (0, 1)), (what, on, any_hit, st)
                    offsets = int(st[1]) == 1
                else:
                    offsets = on and expect_offsets
                    assert (int(st[1]), int(st[0])) == ((1, 0) if offsets else (0, 1)), (what, on, any_hit, st)
                assert gpu.kernel_name(2, top, any_hit).endswith(",true>" if offsets else ",false>"), gpu.kernel_name(2, top, any_hit)
                if octants is not None:
                    assert int(st[3]) >= octants, (what, on, any_hit, st)
    finally:
        gpu.record_offsets(True)
    return refs


@pytest.fixture(scope="module")
def cornell_sets(cornell):
    return {"primary": F.read_rays(cornell.bvh_path.parent / "cornell-primary-64x64.rays", 0.0, 5000.0),
        "random": F.read_rays(cornell.bvh_path.parent / "cornell-random-4096.rays", 0.0, 1.0)}


@pytest.fixture(scope="module")
def cornell_refs(oracle, cornell, cornell_sets):
    nodes, tris = cornell.blocks[2]
    return {name: {any_hit: oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)[0] for any_hit in (False, True)}
        for name, rays in cornell_sets.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("rays", ["primary", "random"])
def test_parity_in_both_forms_and_the_fallback(gpu, oracle, cornell, cornell_sets, cornell_refs, rays):
    """The Cornell goldens, closest and any hit, switch on and off: the oracle's bytes; with the switch off -- and where the allocator put
    the two arrays out of the offset form's reach -- stats[0] reports the 64-bit form."""
    nodes, tris = cornell.blocks[2]
    # one buffer: the offset form certainly applies
    bvh, _ = carve(gpu, nodes, tris, True, 0)
    run_both_forms(gpu, oracle, bvh, nodes, tris, cornell_sets[rays], f"cornell {rays}, one buffer", refs=cornell_refs[rays])
    # the package's own loader keeps both arrays in one allocation: the offset form, whatever the allocator does
    own = gpu.DeviceBvh(2, nodes, tris, 0)
    assert own.nodes.data_ptr() == own.buffer.data_ptr() and own.tris.data_ptr() % 256 == 0
    assert 0 < own.tris.data_ptr() - own.nodes.data_ptr() == (own.nodes.numel() + 255) // 256 * 256
    run_both_forms(gpu, oracle, own, nodes, tris, cornell_sets[rays], f"cornell {rays}, DeviceBvh", refs=cornell_refs[rays])
    # two allocations of the caller's: nobody promises where the allocator puts them (they were measured 32.6 GiB apart under a
    # profiler) -- either form may run with the switch on, and says so
    two = gpu.DeviceBvh.from_tensors(2, gpu.to_device(nodes, 0), gpu.to_device(tris, 0), len(nodes), len(tris), 0)
    run_both_forms(gpu, oracle, two, nodes, tris, cornell_sets[rays], f"cornell {rays}, two allocations", expect_offsets=None,
        refs=cornell_refs[rays])


def tiny_scene():
    """One node, two leaves of one triangle each (test_gpu_octant_loops.flat_and_grazing_scene's shape, octant 0): 64 + 96 bytes."""
    nodes, tris = np.zeros(1, F.NODE2), np.zeros(2, F.TRI1)
    for i, z in enumerate((1.0, 3.0)):
        v0, v1, v2 = (np.float32(p) for p in ([-10, -10, z], [30, -10, z], [-10, 30, z]))
        tris[i]["v0"] = v0; tris[i]["e1"] = v0 - v1; tris[i]["e2"] = v2 - v0
        tris[i]["prim_id"] = np.int32(i) | np.int32(-2 ** 31)
    nodes[0]["bounds"] = [-8, 8, -8, 8, 0.5, 1.5] + [-8, 8, -8, 8, 2.5, 3.5]
    nodes[0]["child"] = [~0, ~1]
    return nodes, tris


@pytest.mark.gpu
@pytest.mark.parametrize("nodes_first", [True, False])
@pytest.mark.parametrize("distance", [64, 48 + 64 * 1024, 3 * 1024 * 1024 + 16])
def test_either_array_lower_in_memory(gpu, oracle, cornell, cornell_sets, cornell_refs, nodes_first, distance):
    """Nodes and triangles carved out of one buffer, once nodes first and once triangles first: the base is the lower one, the other's
    distance is positive, and the distance of the nodes' fictitious record 0 wraps below zero when the nodes ARE the base."""
    rng = np.random.default_rng(distance)
    # the tiny tree: start-to-start distances of exactly 64 (nodes first: one node) / 96 (the two triangles first), 48 + 64 k and 3 MiB
    nodes, tris = tiny_scene()
    org = np.zeros((200, 3), np.float32); org[:, :2] = rng.uniform(-9, 9, (200, 2))
    d = np.tile(np.float32([0.0, 0.0, 1.0]), (200, 1)); d[:, :2] = rng.uniform(-0.2, 0.2, (200, 2))
    rays = F.make_rays(org, d, 0.0, 100.0)
    rays["tmin"][::5] = 2.0                                       # past the first triangle
    bvh, got = carve(gpu, nodes, tris, nodes_first, distance)
    assert got == max(distance, 64 if nodes_first else 96)
    refs = run_both_forms(gpu, oracle, bvh, nodes, tris, rays, f"tiny, nodes_first {nodes_first}, distance {got}")
    assert {0, 1, -1} <= set(refs[False]["tri_id"])
    # Cornell: the lower array is longer than 64 bytes, the other one starts `distance` behind its start or right behind its end
    nodes, tris = cornell.blocks[2]
    bvh, got = carve(gpu, nodes, tris, nodes_first, distance)
    run_both_forms(gpu, oracle, bvh, nodes, tris, cornell_sets["random"], f"cornell, nodes_first {nodes_first}, distance {got}",
        refs=cornell_refs["random"])


@pytest.mark.gpu
@pytest.mark.parametrize("nodes_first", [True, False])
def test_top_of_both_arrays(gpu, oracle, nodes_first):
    """A seeded soup of 600 triangles (tests/lbvh_model.py, one triangle per leaf: 599 nodes, more than the LDS image's 255): rays aimed at
    the LAST triangle of the array and through the box of the LAST node, which the kernel fetches from memory; the upper array ends with
    the buffer's last byte; n ragged.  A lane reads bytes 0..47 of a triangle and 0..55 of a node, whatever its form (in the offset form
    the node lanes alone load the child ids): nothing outside the two arrays, whose neighbourhood holds 0xFF bytes here."""
    import lbvh_model
    from rodent_amd import topimage
    from test_collapse_model import plain_soup
    v, ix = plain_soup(600, 7)
    nodes, tris, _ = lbvh_model.build(v, ix, max_leaf=1)
    nodes, tris = np.frombuffer(nodes.tobytes(), F.NODE2).copy(), np.frombuffer(tris.tobytes(), F.TRI1).copy()
    assert len(nodes) == 599 and len(tris) == 600
    rng = np.random.default_rng(17)
    last = tris[-1]
    v0, e1, e2 = (last[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    n = 64 * 9 + 37
    uv = rng.uniform(0.05, 0.45, (n, 2))
    target = v0 - uv[:, :1] * e1 + uv[:, 1:] * e2                         # v1 = v0 - e1, v2 = v0 + e2
    b = nodes[-1]["bounds"].astype(np.float64)
    target[n // 2:] = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2]) + rng.normal(0, 1e-3, (n - n // 2, 3))
    org = target + rng.normal(0, 1, (n, 3)) * 30.0
    rays = F.make_rays(org.astype(np.float32), (target - org).astype(np.float32), 0.0, 2.0)
    ref, _ = oracle.traverse(2, nodes, tris, rays)
    last_prim = int(tris["prim_id"][-1] & 0x7FFFFFFF)
    assert (tris["prim_id"] & 0x7FFFFFFF == last_prim).sum() == 1 and (ref["tri_id"] == last_prim).sum() >= 32, \
        "rays must end in the array's last triangle"
    assert len(nodes) - 1 not in set(int(i) for i in topimage.image_nodes(nodes)), "the last node must come from memory"
    assert oracle.node_visits(nodes, tris, rays)[len(nodes) - 1] > 0, "rays must pass the last node"
    for count in (n, 64 * 3, 1):
        bvh, _ = carve(gpu, nodes, tris, nodes_first, 0, tail=0)
        run_both_forms(gpu, oracle, bvh, nodes, tris, rays[:count], f"soup, nodes_first {nodes_first}, n {count}")


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [16, 63])
def test_with_the_spill_path(gpu, oracle, depth):
    """conftest.chain_bvh2: stacks of 16 and 63 entries against LDS windows of 15 -- the offset form meets stack_spill / stack_reload."""
    from conftest import chain_bvh2
    nodes, tris = chain_bvh2(depth)
    rng = np.random.default_rng(depth)
    n = 64 * 5 + 11
    org = np.zeros((n, 3), "<f4"); org[:, :2] = rng.uniform(-4, 4, (n, 2)); org[::3, 0] += 50.0
    # one direction: whole chunks; then no common direction or origin: the refill loop
    for name, jitter in (("chunks", 0.0), ("refill", 1e-4)):
        d = np.tile(np.float32([0.001, 0.002, 1.0]), (n, 1)); d[:, :2] += rng.uniform(-jitter, jitter, (n, 2)).astype("<f4")
        rays = F.make_rays(org, d, 0.0, 1000.0)
        ref, st = oracle.traverse(2, nodes, tris, rays)
        assert st["max_stack"] == depth
        bvh, _ = carve(gpu, nodes, tris, False, 4096)
        run_both_forms(gpu, oracle, bvh, nodes, tris, rays, f"chain_bvh2({depth}), {name}")
        gpu.read_stats(0)
        gpu.traverse(bvh, rays, variant=gpu.variants(2).index("top"))
        st = gpu.read_stats(0)
        assert st[7] > 0 and st[1] == 1 and st[5] == (1 if jitter else 0), st


@pytest.mark.gpu
@pytest.mark.parametrize("octant", [0, 5])
def test_with_a_one_octant_tile(gpu, oracle, cornell, octant):
    """Chunks of one origin and one octant take slab_canonical<OCT>'s loop (stats[3]) in either form; with the octant loops off, the
    generic loop."""
    from test_gpu_octant_loops import CORNELL_EYE, octant_dirs
    nodes, tris = cornell.blocks[2]
    rng = np.random.default_rng(octant)
    rays = F.make_rays(np.tile(CORNELL_EYE, (64 * 4 + 9, 1)), octant_dirs(rng, octant, 64 * 4 + 9), 0.0, 100.0)
    bvh, _ = carve(gpu, nodes, tris, True, 0)
    refs = run_both_forms(gpu, oracle, bvh, nodes, tris, rays, f"octant {octant}", octants=1)
    try:
        gpu.octant_loops(False)
        run_both_forms(gpu, oracle, bvh, nodes, tris, rays, f"octant {octant}, generic loop", refs=refs)
    finally:
        gpu.octant_loops(True)
