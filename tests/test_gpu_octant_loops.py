"""One-octant chunks of the default BVH2 kernel (k_bvh2_top_auto; rodent_hip_octant_loops).

A 64-ray chunk whose rays share the three signs of their reciprocal direction -- and have finite origins, directions, idir and oidir --
is traced by the copy of the step loop compiled for that octant, whose slab tests pick the near and the far plane by the known sign
instead of with fminf / fmaxf.  Every other chunk takes the generic loop.  Whichever loop runs, every Hit1 record is the CPU oracle's,
byte for byte (closest hit; any hit: the same records too wherever no NaN is involved, else the same hit / no-hit answers, as in
test_special_tmin_tmax_values), with the switch on and off; stats[3] -- workgroup 0's chunks that took an octant's loop -- says which
loop ran.

Small launches reach the kernel through rodent_hip_top_min_rays(0) and variant "top".  Which chunks workgroup 0 traces follows from the
launch geometry (stripe_rank / ray_of in traversal_top.h): its wave w starts at position w * G * 64 of stripe 0's first 2048 positions,
G = workgroups / 64; nothing in these launches is large enough for a second draw.
"""
import numpy as np
import pytest

from rodent_amd import formats as F

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234664e+38)
SIGNS = [np.float32([-1.0 if o & 1 else 1.0, -1.0 if o & 2 else 1.0, -1.0 if o & 4 else 1.0]) for o in range(8)]


@pytest.fixture(scope="module")
def gpu(native_build):
    import torch
    from rodent_amd import abi
    assert torch.cuda.is_available(), "these tests need a GPU"
    abi.top_min_rays(0)                 # every default launch through k_bvh2_top_auto
    yield abi
    abi.top_min_rays(-1)
    abi.octant_loops(True)


@pytest.fixture(scope="module")
def cornell_dev(gpu, cornell):
    return gpu.DeviceBvh(2, *cornell.blocks[2], 0)


# ---- the host's model of the kernel's decision ---------------------------------------------------------------------------------------

def chunk_octant(rays):
    """chunk_octant (traversal_top.h) for the rays of ONE chunk: the octant all of them share, or -1."""
    with np.errstate(all="ignore"):
        o, d = rays["org"].astype(np.float32), rays["dir"].astype(np.float32)
        idir = np.where(np.abs(d) < np.float32(1e-8), np.copysign(FLT_MAX, d), np.float32(1.0) / d).astype(np.float32)   # safe_rcp
        oidir = (-(o * idir)).astype(np.float32)
    if not all(np.isfinite(x).all() for x in (o, d, idir, oidir)):
        return -1
    neg = np.signbit(idir)
    octs = neg[:, 0] * 1 + neg[:, 1] * 2 + neg[:, 2] * 4
    return int(octs[0]) if (octs == octs[0]).all() else -1


def workgroup0_chunks(gpu, num_chunks):
    """Positions (in chunks) that workgroup 0's sixteen waves trace in a launch of num_chunks chunks (fewer than 8192: first draws only)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = ((cus * 2 + 63) // 64) * 64                    # persistent_groups(32 waves per CU, 16 per workgroup)
    per_stripe = groups // 64
    assert num_chunks < 8192
    ticket = [w * per_stripe for w in range(16)]             # stripe_rank(wave) of workgroup 0, in chunks
    position = [(t // 32) * 64 * 32 + t % 32 for t in ticket]   # ray_of: stripe 0's 32-chunk groups lie 64 groups apart
    return [c for c in position if c < num_chunks]


def expected_count(gpu, rays, chunks=None):
    """stats[3] of one launch with the switch on; chunks: the ray indices of every chunk by position (default: list order)."""
    n = len(rays)
    if chunks is None:
        chunks = [np.arange(c * 64, min(n, c * 64 + 64)) for c in range((n + 63) // 64)]
    return sum(chunk_octant(rays[chunks[c]]) >= 0 for c in workgroup0_chunks(gpu, len(chunks)))


def tiles_of(width, height):
    """Positions -> rays of a recognised image: 8 x 8 tiles over the whole bands of 8 rows, list order behind them (tile_ray)."""
    n, banded = width * height, (height // 8) * 8 * width
    chunks = []
    for tile in range(banded // 64):
        band, tx = divmod(tile, width // 8)
        first = band * 8 * width + tx * 8
        chunks.append(np.array([first + (l >> 3) * width + (l & 7) for l in range(64)]))
    for first in range(banded, n, 64):
        chunks.append(np.arange(first, min(n, first + 64)))
    return chunks


def check(gpu, oracle, bvh, nodes, tris, rays, expect, what, any_bytes=True, chunks=None):
    """Both loops against the oracle, closest and any hit, and the count of either launch.  expect: stats[3] with the switch on (None:
    from the model)."""
    top = gpu.variants(2).index("top")
    if expect is None:
        expect = expected_count(gpu, rays, chunks)
    refs = {any_hit: oracle.traverse(2, nodes, tris, rays, any_hit=any_hit)[0] for any_hit in (False, True)}
    try:
        for on in (True, False):
            gpu.octant_loops(on)
            for any_hit in (False, True):
                gpu.read_stats(0)
                got = gpu.traverse(bvh, rays, any_hit=any_hit, variant=top)
                st = gpu.read_stats(0)
                ref = refs[any_hit]
                if any_hit and not any_bytes:
                    assert np.array_equal(got["tri_id"] >= 0, ref["tri_id"] >= 0), (what, on, any_hit)
                else:
                    bad = np.nonzero((got.view("<u4").reshape(-1, 4) != ref.view("<u4").reshape(-1, 4)).any(axis=1))[0]
                    assert got.tobytes() == ref.tobytes(), (what, on, any_hit, bad[:4], got[bad[:2]], ref[bad[:2]])
                assert int(st[3]) == (expect if on else 0), (what, on, any_hit, int(st[3]), expect)
    finally:
        gpu.octant_loops(True)
    return expect


def octant_dirs(rng, octant, count):
    """Directions spread over one octant (no component near zero)."""
    return (rng.uniform(0.05, 1.0, (count, 3)).astype(np.float32) * SIGNS[octant]).astype(np.float32)


CORNELL_EYE = np.float32([0.13, 0.9, 0.21])             # inside the box, no coordinate zero


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("octant", range(8))
def test_one_origin_chunks_in_every_octant(gpu, oracle, cornell, cornell_dev, octant):
    nodes, tris = cornell.blocks[2]
    rng = np.random.default_rng(octant)
    rays = F.make_rays(np.tile(CORNELL_EYE, (64, 1)), octant_dirs(rng, octant, 64), 0.0, 100.0)
    assert chunk_octant(rays) == octant
    assert check(gpu, oracle, cornell_dev, nodes, tris, rays, 1, f"octant {octant}") == 1
    # one ray of another octant in the chunk: the generic loop, the same records
    for lane, other in ((0, octant ^ 1), (37, octant ^ 6), (63, octant ^ 4)):
        mixed = rays.copy()
        mixed["dir"][lane] = octant_dirs(rng, other, 1)[0]
        check(gpu, oracle, cornell_dev, nodes, tris, mixed, 0, f"octant {octant}, lane {lane} in octant {other}")
    # several chunks of one octant each: workgroup 0 counts its own
    many = F.make_rays(np.tile(CORNELL_EYE, (640, 1)), octant_dirs(rng, octant, 640), 0.0, 100.0)
    assert check(gpu, oracle, cornell_dev, nodes, tris, many, None, f"octant {octant}, 10 chunks") >= 1


def test_zero_and_tiny_direction_components_and_non_finite_lanes(gpu, oracle, cornell, cornell_dev):
    """safe_rcp's branch (|d| < 1e-8: idir = +-FLT_MAX, and with a non-zero origin oidir overflows to +-inf), and NaN / +-inf in one
    lane's origin or direction: the chunk takes the generic loop."""
    nodes, tris = cornell.blocks[2]
    rng = np.random.default_rng(11)
    denormal = np.float32(1e-40)
    # an origin beside the box with every |coordinate| > 1: o * FLT_MAX overflows; and one inside it, where oidir stays finite and the
    # signs of the +-FLT_MAX reciprocals decide like any other (the model says which loop)
    for eye, overflows in ((np.float32([1.5, 1.2, 2.7]), True), (CORNELL_EYE, False)):
        base = F.make_rays(np.tile(eye, (64, 1)), octant_dirs(rng, 4, 64), 0.0, 100.0)
        for value in (np.float32(0.0), np.float32(-0.0), denormal, -denormal, np.float32(1e-9), np.float32(-1e-9)):
            for axis in range(3):
                for lanes in ([5], list(range(64))):
                    rays = base.copy()
                    rays["dir"][lanes, axis] = value
                    if overflows:
                        assert chunk_octant(rays) == -1
                    check(gpu, oracle, cornell_dev, nodes, tris, rays, None, f"eye {eye} dir[{axis}] = {value!r} in lanes {lanes[:2]}")
    base = F.make_rays(np.tile(CORNELL_EYE, (64, 1)), octant_dirs(rng, 4, 64), 0.0, 100.0)
    # the same components from the ORIGIN of coordinates: oidir = -(0 * idir) stays finite, the signs decide (all lanes alike: one octant)
    rays = F.make_rays(np.zeros((64, 3), np.float32), octant_dirs(rng, 4, 64), 0.0, 100.0)
    rays["dir"][:, 0] = np.float32(-0.0)
    assert chunk_octant(rays) == 5
    check(gpu, oracle, cornell_dev, nodes, tris, rays, 1, "origin 0, dir.x = -0 in every lane")
    for field, axis, value in (("org", 0, np.nan), ("org", 2, np.inf), ("org", 1, -np.inf), ("dir", 1, np.nan), ("dir", 0, np.inf),
        ("dir", 2, -np.inf)):
        for lane in (0, 29, 63):
            rays = base.copy()
            rays[field][lane, axis] = np.float32(value)
            assert chunk_octant(rays) == -1
            # (any hit: the answers, as test_special_tmin_tmax_values compares them where a NaN is involved)
            check(gpu, oracle, cornell_dev, nodes, tris, rays, 0, f"{field}[{axis}] = {value} in lane {lane}", any_bytes=False)


def test_ragged_launches_and_padded_lanes(gpu, oracle, cornell, cornell_dev):
    """n % 64 != 0: the padded lanes hold a copy of the chunk's first ray and do not vote."""
    nodes, tris = cornell.blocks[2]
    rng = np.random.default_rng(5)
    for n in (1, 33, 63, 65, 127, 200):
        rays = F.make_rays(np.tile(CORNELL_EYE, (n, 1)), octant_dirs(rng, 2, n), 0.0, 100.0)
        assert check(gpu, oracle, cornell_dev, nodes, tris, rays, None, f"n {n}, one octant") >= 1
    # n = 65: the lone ray of the second chunk is of another octant -- each chunk is decided by its own rays
    rays = F.make_rays(np.tile(CORNELL_EYE, (65, 1)), octant_dirs(rng, 2, 65), 0.0, 100.0)
    rays["dir"][64] = octant_dirs(rng, 5, 1)[0]
    assert check(gpu, oracle, cornell_dev, nodes, tris, rays, None, "n 65, ray 64 in another octant") >= 1
    # ... and the other way round: the first chunk mixed, the one-ray chunk behind it of one octant by itself
    rays["dir"][7] = octant_dirs(rng, 7, 1)[0]
    check(gpu, oracle, cornell_dev, nodes, tris, rays, None, "n 65, first chunk mixed")
    # the last valid lane decides: only lane 32 of a 33-ray chunk differs
    rays = F.make_rays(np.tile(CORNELL_EYE, (33, 1)), octant_dirs(rng, 2, 33), 0.0, 100.0)
    rays["dir"][32] = octant_dirs(rng, 3, 1)[0]
    check(gpu, oracle, cornell_dev, nodes, tris, rays, 0, "n 33, lane 32 in another octant")


def test_images_whose_tiles_straddle_a_sign_boundary(gpu, oracle, cornell, cornell_dev):
    """A camera looking (nearly) along -z: dir.x and dir.y change sign inside the image, in the middle of a tile.  Tiles on one side of both
    boundaries take their octant's loop, the tiles the boundaries cross take the generic one -- both kinds in one launch -- and rows
    behind the last band of 8 are chunks in list order."""
    from rodent_amd import raygen
    nodes, tris = cornell.blocks[2]
    eye, up, fov = (0.03, 1.0, 2.7), (0.0, 1.0, 0.0), 60.0
    for (w, h), look in (((256, 16), (0.004, 0.003, -1.0)), ((136, 24), (0.0, 0.0, -1.0)), ((136, 27), (0.0, 0.0, -1.0)),
        ((256, 21), (0.004, 0.003, -1.0))):
        rays = raygen.primary_rays(eye, look, up, fov, w, h, 0.0, 5000.0)
        chunks = tiles_of(w, h)
        kinds = [chunk_octant(rays[c]) for c in chunks]
        assert any(k < 0 for k in kinds) and len({k for k in kinds if k >= 0}) >= 2, (w, h, kinds)
        gpu.read_stats(0)
        gpu.traverse(cornell_dev, rays, variant=gpu.variants(2).index("top"))
        assert int(gpu.read_stats(0)[2]) == w, "the image was not recognised: the model's tiles are not the kernel's"
        check(gpu, oracle, cornell_dev, nodes, tris, rays, None, f"{w} x {h}", chunks=chunks)


def flat_and_grazing_scene(octant):
    """Two leaves under one root, mirrored into `octant`.  Leaf 0: a box that rays from the origin along s * (1, 1, 0.5) touch in ONE
    point, the edge x = 2, y = 2 (the x slab gives t in [1, 2], the y slab [2, 3]: tentry == texit == 2), with a triangle in the plane z =
    1 there.  Leaf 1: a box with lo == hi on z (an axis-aligned quad in the plane z = 3), which the same rays meet in its corner x = y =
    6, t = 6.  Every number is exact in float32."""
    s = SIGNS[octant]
    nodes, tris = np.zeros(1, F.NODE2), np.zeros(2, F.TRI1)

    def box(x, y, z):
        out = []
        for a, (lo, hi) in zip(s, (x, y, z)):
            out += sorted((float(a * lo), float(a * hi)))
        return out

    for i, z in enumerate((1.0, 3.0)):
        v0, v1, v2 = (np.float32(p) * s for p in ([-10, -10, z], [30, -10, z], [-10, 30, z]))
        tris[i]["v0"] = v0; tris[i]["e1"] = v0 - v1; tris[i]["e2"] = v2 - v0
        tris[i]["prim_id"] = np.int32(i) | np.int32(-2 ** 31)
    nodes[0]["bounds"] = box((1, 2), (2, 3), (-8, 8)) + box((0, 6), (0, 6), (3, 3))
    nodes[0]["child"] = [~0, ~1]
    return nodes, tris


@pytest.mark.parametrize("octant", range(8))
def test_flat_boxes_and_grazing_rays(gpu, oracle, octant):
    nodes, tris = flat_and_grazing_scene(octant)
    bvh = gpu.DeviceBvh(2, nodes, tris, 0)
    s = SIGNS[octant]
    k = np.arange(64)
    d = np.tile(np.float32([1.0, 1.0, 0.5]), (64, 1))
    d *= (np.float32(2.0) ** (k % 8 - 4))[:, None]                       # the same line at other speeds: still exact
    d[k >= 32, 1] += (np.float32(2.0) ** -20) * ((k[k >= 32] % 5) - 2)    # ... and just beside the edge, on both sides
    rays = F.make_rays(np.zeros((64, 3), np.float32), (d * s).astype(np.float32), 0.0, 100.0)
    assert chunk_octant(rays) == octant
    ref = oracle.traverse(2, nodes, tris, rays)[0]
    # the grazing rays hit the triangle of the box they only touch; beside the edge some miss it
    assert (ref["tri_id"][:32] == 0).all() and set(ref["tri_id"][32:]) >= {0, 1}
    check(gpu, oracle, bvh, nodes, tris, rays, 1, f"graze, octant {octant}")
    # past the first triangle (tmin behind it): the flat box's corner, tentry == texit == 6 on a box with lo == hi
    far = rays.copy()
    far["tmin"] = (np.float32(2.5) / np.abs(far["dir"][:, 0])).astype(np.float32)
    ref = oracle.traverse(2, nodes, tris, far)[0]
    assert (ref["tri_id"][:32] == 1).all()
    check(gpu, oracle, bvh, nodes, tris, far, 1, f"flat box, octant {octant}")


def test_special_tmin_tmax_values_in_one_octant_chunks(gpu, oracle, cornell, cornell_dev):
    """The twelve special values of test_special_tmin_tmax_values, every pair of them, in chunks of one origin and one octant: the
    specialised loops keep the two raw v_max / v_min against the canonical bounds."""
    nodes, tris = cornell.blocks[2]
    specials = np.array([0x00000000, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345,
                         0x40A00000, 0xBF800000, 0x3C23D70A, 0x7F7FFFFF], dtype="<u4").view("<f4")
    n = len(specials) ** 2
    rng = np.random.default_rng(3)
    k = np.arange(n)
    for octant in (0, 3, 6):
        rays = F.make_rays(np.tile(CORNELL_EYE, (n, 1)), octant_dirs(rng, octant, n), 0.0, 100.0)
        rays["tmin"] = specials[k % len(specials)]
        rays["tmax"] = specials[k // len(specials)]
        assert check(gpu, oracle, cornell_dev, nodes, tris, rays, None, f"special tmin / tmax, octant {octant}", any_bytes=False) >= 1


def test_spill_and_reload_inside_a_specialised_loop(gpu, oracle):
    """conftest.chain_bvh2(40): the stack outgrows the lane's LDS window and comes back (stats[7]: blocks moved out) while the chunk runs
    its octant's loop."""
    from conftest import chain_bvh2
    nodes, tris = chain_bvh2(40)
    bvh = gpu.DeviceBvh(2, nodes, tris, 0)
    rng = np.random.default_rng(40)
    top = gpu.variants(2).index("top")
    for octant, z0 in ((0, -1.0), (3, -1.0)):
        d = np.ones((128, 3), np.float32)
        d[:, :2] = rng.uniform(0.0005, 0.004, (128, 2)).astype(np.float32) * SIGNS[octant][:2]
        rays = F.make_rays(np.tile(np.float32([0.25, -0.5, z0]), (128, 1)), d, 0.0, 1000.0)
        assert chunk_octant(rays[:64]) == octant
        ref, st = oracle.traverse(2, nodes, tris, rays)
        assert st["max_stack"] == 40 and (ref["tri_id"] == 0).all()
        assert check(gpu, oracle, bvh, nodes, tris, rays, None, f"chain_bvh2(40), octant {octant}") >= 1
        gpu.read_stats(0)
        gpu.traverse(bvh, rays, variant=top)
        st = gpu.read_stats(0)
        assert st[3] >= 1 and 0 < st[7] <= 4 * len(rays), st
