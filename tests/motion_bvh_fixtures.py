"""The shapes, times and rays that tests/test_motion_bvh_model.py (CPU) and tests/test_gpu_motion_bvh.py share, and the conditions they
must meet so that no GPU test passes vacuously (check_conditions; the CPU test runs them on the model alone).

Shapes: the Cornell box (tests/golden/cornell_box.obj) with the committed ray sets -- 64 x 64 primary rays, 4096 random segments, the
hand-made edge rays -- and a seeded soup of 2000 triangles with 4096 seeded segments.  Key 1 of either is key 0 under a seeded smooth
displacement (a sine wave per axis along another axis, refit_model.deform's kind; AMPLITUDE of the mesh's extent) plus a seeded
per-vertex jitter of a fifth of that, which tears shared edges apart: a ray can then hit at one key and miss at the other.
"""
from __future__ import annotations

import numpy as np

import motion_bvh_model as MB
from rodent_amd import formats as F

F32 = np.float32
DENORMAL = F32(1e-40)
REFUSED = np.array([np.nan, np.inf, -np.inf, -(2.0 ** -149), np.nextafter(F32(1), F32(2)), -0.25, 1.5], F32)
TRACED_FIXED = np.array([0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24, DENORMAL, -0.0], F32)
# The displacement of each shape: its amplitude as a share of the mesh's extent, and its seed.  Chosen so that the model alone meets
# check_conditions (with the Cornell box's first seed tried no edge ray hit at one key only).
AMPLITUDE = {"cornell": 0.12, "soup": 0.12}
SEED = {"cornell": 1037, "soup": 3000}


def palette(seed=17):
    """The 16 times of the trace tests: the 7 refused ones, the 7 fixed traced ones and 2 seeded ones in (0, 1)."""
    p = np.concatenate([TRACED_FIXED, REFUSED, np.random.default_rng(seed).uniform(0.0, 1.0, 2).astype(F32)])
    assert len(set(p.view("<u4").tolist())) == 16
    return p


def times_for(n):
    """The palette cycled over n rays, starting with a traced time."""
    return palette()[np.arange(n) % 16]


def displace(vertices, seed, amplitude):
    """Key 1 of the (n, 4) float32 vertices: the smooth displacement plus the jitter."""
    rng = np.random.default_rng(seed)
    v = np.array(vertices, F32).reshape(-1, 4).copy()
    p = v[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    extent = max(float((hi - lo).max()), 1e-3)
    freq = rng.uniform(1.0, 3.0, 3) * 2 * np.pi / extent
    phase = rng.uniform(0, 2 * np.pi, 3)
    amp = amplitude * extent * rng.uniform(0.5, 1.0, 3)
    jitter = rng.uniform(-0.2, 0.2, p.shape) * amplitude * extent
    for a in range(3):
        v[:, a] = (p[:, a] + amp[a] * np.sin(freq[a] * p[:, (a + 1) % 3] + phase[a]) + jitter[:, a]).astype(F32)
    return v


def soup_mesh(n=2000, seed=23):
    """n triangles with corners of their own, no two alike, large enough that a quarter of the segments below hit one."""
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 4), F32)
    centre = rng.uniform(-50, 50, (n, 1, 3))
    v[:, :3] = (centre + rng.uniform(-9, 9, (n, 3, 3))).reshape(-1, 3).astype(F32)
    ix = np.zeros((n, 4), np.int32)
    ix[:, :3] = np.arange(3 * n).reshape(n, 3)
    ix[:, 3] = rng.integers(0, 5, n)
    return v, ix


def segments(lo, hi, n, seed):
    """n seeded segments between points of the box [lo, hi]: tmin 0, tmax 1."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(lo, hi, (n, 3)), rng.uniform(lo, hi, (n, 3))
    return F.make_rays(a.astype(F32), (b - a).astype(F32), 0.0, 1.0)


class Shape:
    """One mesh at its two keys with its ray classes {name: rays}."""

    def __init__(self, name, vertices, indices, rays):
        self.name, self.ix, self.rays = name, np.asarray(indices, np.int32).reshape(-1, 4), rays
        self.v0 = np.array(vertices, F32).reshape(-1, 4)
        self.v1 = displace(self.v0, SEED[name], AMPLITUDE[name])

    def records(self, nodes, tris):
        """The model's motion records over the topology nodes / tris."""
        mn, mt, info = MB.build(nodes, tris, self.v0, self.v1, self.ix)
        assert info.tolist() == [len(nodes), len(nodes) + len(tris), 0, len(nodes)], (self.name, info)
        return mn, mt


def shapes(cornell_scene, cornell):
    """[Shape]: `cornell_scene` is the converted tests/golden/cornell_box.obj (rodent_amd.scene), `cornell` conftest's fixture."""
    box = Shape("cornell", cornell_scene.vertices, cornell_scene.indices, {k: cornell.ray_sets[k] for k in ("primary", "random", "edge")})
    v, ix = soup_mesh()
    return [box, Shape("soup", v, ix, {"segments": segments(v[:, :3].min(0), v[:, :3].max(0), 4096, 29)})]


def check_conditions(oracle, shape, mn, mt):
    """The conditions, per ray class, on the model alone; returns {class: (hit share, share that differs from both keys, rays that hit
    at one key only)} for the caller to print."""
    out = {}
    for name, rays in shape.rays.items():
        n = len(rays)
        times = times_for(n)
        hits = MB.trace(oracle, mn, mt, rays, times)
        on = MB.traced(times)
        share = float((hits["tri_id"][on] >= 0).mean())
        assert share >= 0.25, (shape.name, name, share)
        assert (hits["tri_id"][~on] == -1).all()
        h0, h1, hm = (MB.trace(oracle, mn, mt, rays, np.full(n, t, F32)) for t in (0.0, 1.0, 0.5))
        hit = hm["tri_id"] >= 0
        differs = lambda a: (a["tri_id"] != hm["tri_id"]) | (a["t"] != hm["t"])
        moved = float((differs(h0) & differs(h1))[hit].mean())
        assert moved >= 0.10, (shape.name, name, moved)
        flipped = int(((h0["tri_id"] >= 0) != (h1["tri_id"] >= 0)).sum())
        assert flipped >= 1, (shape.name, name)
        out[name] = (share, moved, flipped)
    return out
