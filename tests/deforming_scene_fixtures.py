"""The scene, the keys and the crafted trace sets that tests/test_deforming_scene_model.py (CPU) and tests/test_gpu_deforming_render.py
share, and the conditions they must meet so that no GPU test passes vacuously (check_conditions; the CPU test runs them on the model
alone).

Scene: tests/golden/cornell_box.obj with one two-sided quad (two triangles) added above the boxes.  Key 1 moves only the vertices of
shortBox and tallBox -- a seeded shear of both plus a twist of the tall box about y, the short box sliding by about its width -- and
turns the quad by 155 degrees about the vertical axis through its centre, so that it shows its other side at time 1 and turns over in
between.  Every wall and the light keep their bytes.  Film 32 x 24, 2 spp, paths of 4, shutters (0, 1) and (0.25, 0.75).
"""
from __future__ import annotations

import shutil

import numpy as np

import deforming_scene_model as DM
import lbvh_model as L
import motion_bvh_model as MB
from oracle import binding as O
from rodent_amd import formats as F
from shade_fixtures import FLT_MAX_REF, RAY_OFFSET, SHADOW_TMAX

F32 = np.float32
W, H, SPP, MAXLEN = 32, 24, 2, 4
SHUTTERS = ((0.0, 1.0), (0.25, 0.75))
SEED = 11
# key 0: a canopy under the light that rises towards the back, its upper side towards the camera.  (Placed and turned so that the
# model alone meets check_conditions under both shutters: a smaller quad, or one turned by 170 degrees, which is all but edge-on around
# t = 0.5, left fewer than a quarter of the shadow rays occluded.)
QUAD = ((-0.75, 1.5, 0.65), (0.75, 1.5, 0.65), (0.75, 1.72, -0.65), (-0.75, 1.72, -0.65))
QUAD_TURN = np.radians(155.0)
SLIDE = -0.55                                                                           # the short box, along x: about its width
QUAD_ORIGIN = (0.0, 1.5, 2.5)


class Parts:
    """scene (key 0, converted), keys (deforming_scene_model.Keys), topology (nodes, tris: lbvh_model.build of key 0 at max_leaf 2, as
    the scene's default build writes it), the vertex sets `short`, `tall`, `quad` and the triangle sets `box_tris`, `quad_tris`."""


def parts(golden, tmp):
    from rodent_amd import scene as S
    text = (golden / "cornell_box.obj").read_text()
    n = sum(1 for line in text.splitlines() if line.split()[:1] == ["v"])
    text += ("\n## the turning quad\nusemtl shortBox\n" + "".join("v %g %g %g\n" % q for q in QUAD)
             + f"f {n + 1} {n + 2} {n + 3}\nf {n + 1} {n + 3} {n + 4}\n")
    (tmp / "deforming.obj").write_text(text)
    shutil.copy(golden / "cornell_box.mtl", tmp / "cornell_box.mtl")
    p = Parts()
    p.scene = S.convert(tmp / "deforming.obj", tmp / "deforming.rscene")
    v0 = np.array(p.scene.vertices, F32).reshape(-1, 4)
    ix = np.asarray(p.scene.indices).reshape(-1, 4)
    x, y, z = v0[:, 0], v0[:, 1], v0[:, 2]
    p.quad = np.flatnonzero((v0[:, None, :3] == F32(QUAD)[None]).all(2).any(1))
    on_quad = np.isin(np.arange(len(v0)), p.quad)
    box = (np.abs(x) < 0.9) & (y < 1.25) & ~on_quad
    # (the footprints of the two boxes lie on either side of the line x + z = 0.04)
    p.tall, p.short = np.flatnonzero(box & (x + z < 0.04)), np.flatnonzero(box & (x + z >= 0.04))
    p.box_tris = np.flatnonzero(np.isin(ix[:, :3], np.concatenate([p.tall, p.short])).all(1))
    p.quad_tris = np.flatnonzero(np.isin(ix[:, :3], p.quad).all(1))
    assert len(p.box_tris) == 24 and len(p.quad_tris) == 2 and len(p.quad) >= 4, (len(p.box_tris), len(p.quad_tris), len(p.quad))
    v1 = key1(p, v0)
    p.keys = DM.Keys(v0, v1, p.scene.normals, SU_smooth(v1, ix))
    nodes, tris, info = L.build(v0, ix, 2)
    assert info[2] == 0
    p.topology = (nodes, tris)
    fixed = np.setdiff1d(np.arange(len(v0)), np.concatenate([p.tall, p.short, p.quad]))
    assert v1[fixed].tobytes() == v0[fixed].tobytes() and not DM.moving_light(p.scene, v1)
    return p


def SU_smooth(vertices, indices):
    import scene_update_model as SU
    return SU.smooth_normals(SU.face_normals(vertices, indices), indices, len(vertices))


def key1(p, v0, seed=SEED):
    """Key 1 of the vertices: seeded, in float64, rounded once."""
    rng = np.random.default_rng(seed)
    v1 = v0.copy()
    q = v0[:, :3].astype(np.float64)
    shear = rng.uniform(0.15, 0.3, 2) * rng.choice([-1.0, 1.0], 2)
    # the tall box: x += k y, then a twist about the vertical axis through its centre that grows with the height
    t = q[p.tall]
    c = t.mean(0)
    angle = 0.9 * t[:, 1] / max(t[:, 1].max(), 1e-6)
    dx, dz = t[:, 0] - c[0], t[:, 2] - c[2]
    t[:, 0] = c[0] + np.cos(angle) * dx + np.sin(angle) * dz + shear[0] * t[:, 1]
    t[:, 2] = c[2] - np.sin(angle) * dx + np.cos(angle) * dz
    v1[p.tall, :3] = t.astype(F32)
    # the short box: slides along x and leans along z
    s = q[p.short]
    s[:, 0] += SLIDE
    s[:, 2] += shear[1] * s[:, 1]
    v1[p.short, :3] = s.astype(F32)
    # the quad: QUAD_TURN about the vertical axis through its centre
    g = q[p.quad]
    c = g.mean(0)
    dx, dz = g[:, 0] - c[0], g[:, 2] - c[2]
    g[:, 0] = c[0] + np.cos(QUAD_TURN) * dx + np.sin(QUAD_TURN) * dz
    g[:, 2] = c[2] - np.sin(QUAD_TURN) * dx + np.cos(QUAD_TURN) * dz
    v1[p.quad, :3] = g.astype(F32)
    return v1


def moved_keys(p, seed=29):
    """(vertices0, vertices1) of an update: both keys somewhere else -- the boxes and the quad displaced by a seeded offset per key; the
    walls and the light keep their bytes."""
    rng = np.random.default_rng(seed)
    out = []
    movers = np.concatenate([p.tall, p.short, p.quad])
    for k in (p.keys.vertices0, p.keys.vertices1):
        v = k.copy()
        v[movers, :3] = (v[movers, :3].astype(np.float64) + rng.uniform(-0.06, 0.06, 3) * np.array([1.0, 0.0, 1.0])
                         + rng.uniform(0.0, 0.04, (len(movers), 1)) * np.array([0.0, 1.0, 0.0])).astype(F32)
        out.append(v)
    return out


def camera():
    from rodent_amd import scene as S
    return S.camera_settings((0, 1, 2.7), (0, 0, -1), (0, 1, 0), 60, W, H)


def seeded_rays(p, seed=5):
    """(rays RAY1, ubits): fans of rays from in front of the scene towards the tall box, the short box at either key and the quad (those
    from QUAD_ORIGIN), each ray four times: at ubits 0, 2^22, 2^23 - 1 and a seeded value; and rays that leave through the open front."""
    rng = np.random.default_rng(seed)
    org, d = [], []
    targets = [p.keys.vertices0[p.tall, :3].mean(0), p.keys.vertices0[p.short, :3].mean(0), p.keys.vertices1[p.short, :3].mean(0),
               p.keys.vertices1[p.tall, :3].mean(0)]
    for k, target in enumerate(targets):
        for j in range(8):
            o = np.array([0.3 * np.cos(j + k), 1.0 + 0.05 * j, 2.5])
            org.append(o); d.append(target.astype(np.float64) + 0.12 * np.array([np.sin(3 * j), np.cos(5 * j), 0.0]) - o)
    for j in range(12):
        org.append(np.array(QUAD_ORIGIN)); d.append(np.array([0.05 * (j % 4 - 1.5), 0.06 * (j // 4 - 1), 0.3]) + (0, 1.5, 0) - QUAD_ORIGIN)
    for j in range(5):                                                   # (49 rays, 196 with their four times: no whole wave)
        org.append((0.0, 1.0, 2.7)); d.append((0.3 * j, 5.0 + j, 1.0))
    n = len(org)
    rays = F.make_rays(np.tile(F32(org), (4, 1)), np.tile(F32(d), (4, 1)), 0.0, FLT_MAX_REF)
    ubits = np.concatenate([np.zeros(n), np.full(n, 1 << 22), np.full(n, (1 << 23) - 1), rng.integers(0, 1 << 23, n)]).astype(np.int32)
    return rays, ubits


def model_frame(p, shutter, keys=None):
    return DM.frame(p.scene, p.keys if keys is None else keys, p.topology, camera(), 0, SPP, MAXLEN, W, H, shutter=shutter)


def ray_classes(p, frame, shutter):
    """{class: (rays, times, any_hit)}: the frame's camera, bounce and shadow rays, and the seeded rays."""
    seeded, su = seeded_rays(p)
    bounce = [t for t in frame.primary[1:]]
    return {"camera": (frame.primary[0][0], DM.shutter_time(frame.primary[0][3], *shutter), False),
            "bounce": (np.concatenate([t[0] for t in bounce]), DM.shutter_time(np.concatenate([t[3] for t in bounce]), *shutter), False),
            "shadow": (np.concatenate([t[0] for t in frame.shadow]), np.concatenate([t[4] for t in frame.shadow]), True),
            "seeded": (seeded, DM.shutter_time(su, *shutter), False)}


def check_conditions(p, frame, shutter=(0.0, 1.0)):
    """The conditions on the model alone; returns the figures for the caller to print."""
    out = {}
    mn, mt = frame.nodes, frame.tris
    for name, (rays, times, any_hit) in ray_classes(p, frame, shutter).items():
        hits = MB.trace(O, mn, mt, rays, times, any_hit)
        out[name] = float((hits["tri_id"] >= 0).mean())
        assert out[name] >= 0.25, (name, out[name])
    # camera hits on a box: the face normal at the hit's time differs from both keys' face normals
    v, _, prims, ubits = frame.vertices[0]
    times = DM.shutter_time(ubits, *shutter)
    on_box = np.isin(prims, p.box_tris)
    at = DM.bake_hits(p.scene, p.keys, frame.lights, prims[on_box], times[on_box]).face_normals
    k0, k1 = (DM.bake_hits(p.scene, p.keys, frame.lights, prims[on_box], np.full(int(on_box.sum()), t, F32)).face_normals for t in (0, 1))
    differs = (at.view("<u4") != k0.view("<u4")).any(1) & (at.view("<u4") != k1.view("<u4")).any(1)
    out["face normal differs from both keys"] = float(differs.mean())
    assert on_box.sum() > 50 and differs.mean() >= 0.10, differs.mean()
    # a camera ray that hits a box at its own time and misses it at key 0, and the reverse
    rays, _, hits, ubits = frame.primary[0]
    own = np.isin(hits["tri_id"], p.box_tris)
    at0 = np.isin(MB.trace(O, mn, mt, rays, np.zeros(len(rays), F32))["tri_id"], p.box_tris)
    out["box at its own time only / at key 0 only"] = (int((own & ~at0).sum()), int((~own & at0).sum()))
    assert (own & ~at0).any() and (~own & at0).any()
    # the turning quad from one origin: both sides
    seeded, su = seeded_rays(p)
    st = DM.shutter_time(su, *shutter)
    sh = MB.trace(O, mn, mt, seeded, st)
    on_quad = np.isin(sh["tri_id"], p.quad_tris) & (seeded["org"] == F32(QUAD_ORIGIN)).all(1)
    entering = quad_entering(p, frame, seeded[on_quad], sh[on_quad], st[on_quad])
    out["quad hits entering / leaving"] = (int(entering.sum()), int((~entering).sum()))
    assert entering.any() and (~entering).any()
    # the wrong face-normal rule is detectable: at least one shaded hit's result differs under it
    out["hits whose shading differs under the wrong rule"] = sum(int(wrong_rule_differs(p, frame, b, shutter).sum())
                                                                 for b in range(len(frame.vertices)))
    assert out["hits whose shading differs under the wrong rule"] >= 1
    return out


def wrong_rule_differs(p, frame, bounce, shutter):
    """Per shaded hit of that bounce: whether the flat oracle's record differs under "face normal = normalised lerp of the keys' face
    normals"."""
    v, _, prims, ubits = frame.vertices[bounce]
    times = DM.shutter_time(ubits, *shutter)
    right = O.shade_vertices(DM.bake_hits(p.scene, p.keys, frame.lights, prims, times), v.copy(), MAXLEN)
    wrong = O.shade_vertices(DM.bake_hits(p.scene, p.keys, frame.lights, prims, times, face_rule="lerp"), v.copy(), MAXLEN)
    return (right.view(np.uint8).reshape(len(v), -1) != wrong.view(np.uint8).reshape(len(v), -1)).any(1)


def quad_entering(p, frame, rays, hits, times):
    """`entering` of the flat shader for hits on the quad: dot(dir, fn) <= 0 with the face normal at the hit's time."""
    fn = DM.bake_hits(p.scene, p.keys, frame.lights, hits["tri_id"], times).face_normals[:, :3]
    d = rays["dir"]
    return (d[:, 0] * fn[:, 0] + d[:, 1] * fn[:, 1] + d[:, 2] * fn[:, 2]) <= 0


def vertices_of_rays(rays, hits, seed=3):
    """ORACLE_VERTEX records for crafted hits (prim to be set by the caller): a seeded random state and a unit contribution."""
    rng = np.random.default_rng(seed)
    v = np.zeros(len(rays), O.ORACLE_VERTEX)
    v["org"], v["dir"] = rays["org"], rays["dir"]
    v["t"], v["u"], v["v"] = hits["t"], hits["u"], hits["v"]
    v["rnd"] = rng.integers(1, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    v["contrib"] = 1.0
    return v
