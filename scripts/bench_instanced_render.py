#!/usr/bin/env python
"""A forest rendered as an instanced scene and as the same geometry baked flat.

usage: python scripts/bench_instanced_render.py [--object plant/1] [--instances 64] -o profiles/gpu_instanced_render.txt

Scene: DESIGN 11's forest -- N seeded placements (scripts/bench_instances.py: layout) of ONE generated plant, diffuse -- over a diffuse
ground quad and under one emissive quad as large as the layout.  Instanced: three objects, N + 2 instances
(render.Renderer(instances=...)); flat: every instance's triangles in world space, its hierarchy built on the device (gpu_bvh=2), through
the renderer's default configuration (mapping "auto").  Both render one frame size and spp from one camera above the layout.  Reported:
the frame, the device bytes, and what moving the copies costs -- set_transforms against update_geometry_device of the flat scene on
vertices that already lie in its own table.  HIP events, ms, median [min, max] of 20 after 3 warm-ups.  Each step is a child process
under its own time limit; the first failure ends the run.
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from bench_instances import REPS, WARMUP, layout, object_mesh, spread, timed             # noqa: E402
from rodent_amd import formats as F, scene as S                                           # noqa: E402

WIDTH, HEIGHT, SPP, MAXLEN = 1024, 576, 4, 8
STEPS = (("instanced", 600), ("flat", 900))


def face_normals(v, ix):
    p = v[:, :3].astype(np.float64)
    c = np.cross(p[ix[:, 1]] - p[ix[:, 0]], p[ix[:, 2]] - p[ix[:, 0]])
    n = np.zeros((len(ix), 4), np.float32)
    n[:, :3] = c / np.maximum(np.linalg.norm(c, axis=1), 1e-30)[:, None]
    return n


def part(v, ix, material, emissive=False):
    """A scene.Scene-like object of one mesh with one material: flat shading normals, one light per triangle if it emits."""
    fn = face_normals(v, ix)
    normals = np.zeros((len(v), 4), np.float32)
    normals[ix[:, :3].reshape(-1)] = np.repeat(fn, 3, axis=0)
    lights = np.zeros(len(ix) if emissive else 0, S.LIGHT)
    if emissive:
        p = v[:, :3].astype(np.float64)
        for k, name in enumerate(("v0", "v1", "v2")):
            lights[name][:, :3] = v[ix[:, k], :3]
        area = 0.5 * np.linalg.norm(np.cross(p[ix[:, 1]] - p[ix[:, 0]], p[ix[:, 2]] - p[ix[:, 0]]), axis=1)
        lights["n"], lights["inv_area"], lights["color"] = fn[:, :3], 1.0 / area, (14.0, 13.0, 11.0, 0.0)
    ix = ix.copy(); ix[:, 3] = 0
    return SimpleNamespace(vertices=v, normals=normals, face_normals=fn, indices=ix, materials=material, lights=lights,
                           light_ids=np.arange(len(ix), dtype=np.int32) if emissive else np.zeros(len(ix), np.int32),
                           texcoords=np.zeros((len(v), 4), np.float32), textures=np.zeros(0, S.TEXTURE), texels=np.zeros(0, np.uint32),
                           nodes=np.zeros(0, F.NODE2), tris=np.zeros(0, F.TRI1), num_tris=len(ix))


def material(kd, emissive=False):
    m = np.zeros(1, S.MATERIAL)
    m["kd"], m["type"], m["emissive"] = kd, (0 if emissive else 1), int(emissive)
    return m


def quad(facing_up):
    v = np.zeros((4, 4), np.float32)
    v[:, :3] = [(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)]
    order = [(0, 2, 1), (0, 3, 2)] if facing_up else [(0, 1, 2), (0, 2, 3)]
    ix = np.zeros((2, 4), np.int32); ix[:, :3] = order
    return v, ix


def forest(a):
    """(objects, transforms, object ids, camera) of the forest."""
    v, ix = object_mesh(a.object)
    t = layout(v, a.instances)
    lo, hi = v[:, :3].min(0), v[:, :3].max(0)
    centres = t.reshape(-1, 3, 4)[:, :, 3]
    span = float(np.ptp(centres[:, [0, 2]], axis=0).max() + 2.0 * np.linalg.norm(hi - lo))
    mid = (centres.min(0) + centres.max(0)) / 2
    def placed(scale, y):
        m = np.zeros((3, 4)); m[0, 0] = m[2, 2] = scale; m[1, 1] = 1.0; m[:, 3] = (mid[0], y, mid[2])
        return m.reshape(12)
    transforms = np.concatenate([t, [placed(span, 1.3 * hi[1] + 0.25 * span),
                                     placed(1.5 * span, min(1.3 * lo[1], 0.7 * lo[1]) - 1e-3 * span)]])
    objects = [part(v, ix, material((0.25, 0.55, 0.2))), part(*quad(False), material((0, 0, 0), True), True),
               part(*quad(True), material((0.5, 0.5, 0.5)))]
    ids = np.concatenate([np.zeros(a.instances, np.int32), [1, 2]]).astype(np.int32)
    eye = mid + np.float32([0.0, 0.35, 0.6]) * span
    cam = S.camera_settings(eye, (mid[0], 0.5 * hi[1], mid[2]) - eye, (0, 1, 0), 50.0, WIDTH, HEIGHT)
    return objects, transforms.astype(np.float32), ids, cam


def baked(scene, ranges, transforms, ids):
    """The forest as one flat scene.Scene-like object: every instance's triangles in world space (fp64 maps, rounded once)."""
    m = transforms.reshape(-1, 3, 4).astype(np.float64)
    vs, ixs = [], []
    nv = 0
    for k, o in enumerate(ids):
        first, n = ranges[o, 0], ranges[o, 1]
        ix = scene.indices[first:first + n]
        used = np.unique(ix[:, :3])
        remap = np.zeros(len(scene.vertices), np.int64); remap[used] = np.arange(len(used))
        w = np.zeros((len(used), 4), np.float32)
        w[:, :3] = scene.vertices[used, :3].astype(np.float64) @ m[k, :, :3].T + m[k, :, 3]
        out = np.zeros((n, 4), np.int32)
        out[:, :3] = remap[ix[:, :3]] + nv; out[:, 3] = ix[:, 3]
        vs.append(w); ixs.append(out); nv += len(used)
    v, ix = np.concatenate(vs), np.concatenate(ixs)
    flat = part(v, ix, scene.materials)
    flat.indices = ix
    glow = scene.materials["emissive"][ix[:, 3]] != 0
    lit = part(v, ix[glow], scene.materials, True)
    flat.lights = lit.lights
    flat.light_ids = np.zeros(len(ix), np.int32); flat.light_ids[glow] = np.arange(int(glow.sum()))
    return flat


def step(name, a):
    import torch
    from rodent_amd import instances as I, render as R
    objects, transforms, ids, cam = forest(a)
    scene = I.concat_scenes(objects)
    stream = torch.cuda.current_stream()
    free0 = torch.cuda.mem_get_info()[0]
    out = {"object_tris": objects[0].num_tris, "instances": len(ids)}
    if name == "instanced":
        r = R.Renderer(scene, WIDTH, HEIGHT, SPP, MAXLEN, instances=(scene.ranges, transforms, ids))
        t_dev = torch.from_numpy(transforms).cuda()
        move = lambda: r.set_transforms(t_dev, check=False)
        out["tlas_nodes"] = int(r.transforms_status()[1][0])
    else:
        flat = baked(scene, scene.ranges, transforms, ids)
        out["flat_tris"] = flat.num_tris
        r = R.Renderer(flat, WIDTH, HEIGHT, SPP, MAXLEN, mapping="auto", gpu_bvh=2)
        tables = r.scene_table_pointers()
        move = lambda: r.update_geometry_device(tables["vertices"], tables["normals"], check=False)
    torch.cuda.synchronize()
    out["scene_bytes"] = int(free0 - torch.cuda.mem_get_info()[0])                  # everything the scene holds, before any stream exists
    nodes, tris, nn, nt = R.vp(), R.vp(), R.i32(), R.i32()
    R.lib().rodent_hip_scene_bvh(0, nodes, tris, nn, nt)
    out["hierarchy_bytes"] = nn.value * F.NODE2.itemsize + nt.value * F.TRI1.itemsize \
        + (out.get("tlas_nodes", 0) * F.NODE2.itemsize + len(ids) * F.INSTANCE.itemsize if name == "instanced" else 0)
    frame = [0]
    def one_frame():
        r.render_rows(cam, frame[0], 0, HEIGHT); frame[0] += 1
    out["frame_ms"] = timed(one_frame, stream)
    c = r.counters()
    out["rays"] = [int(c["primary_rays"]), int(c["shadow_rays"])]
    out["options"] = r.options_in_effect(); out["kernel"] = r.trace_kernel_name()
    out["film_mean"] = float(r.film().mean() / (WARMUP + REPS))
    out["move_ms"] = timed(move, stream)
    out["move_status"] = r.transforms_status()[0] if name == "instanced" else r.update_status()[0]
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--object", default="plant/1", help="scenes.py's generated kind / detail (plant/1, crown/1)")
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one step and print its figures as JSON")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a)))
        return 0
    r = {}
    for name, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, __file__, "--object", a.object, "--instances", str(a.instances), "--step", name],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name} failed (no result within {limit} s): nothing further is run", file=sys.stderr)
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout + p.stderr, file=sys.stderr)
            print(f"step {name} failed (exit status {p.returncode}): nothing further is run", file=sys.stderr)
            return 1
        r[name] = json.loads(line[0][7:])
    inst, flat = r["instanced"], r["flat"]
    ratio = lambda a, b: np.median(a) / np.median(b)
    lines = [f"# scripts/bench_instanced_render.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of "
             f"{REPS} after {WARMUP} warm-ups; {WIDTH} x {HEIGHT}, {SPP} spp, path length <= {MAXLEN}.",
             f"scene: {inst['object_tris']} triangles x {a.instances} placements + ground + light = {flat['flat_tris']} triangles flat, "
             f"{inst['instances']} instances (TLAS: {inst['tlas_nodes']} nodes)",
             f"{'':34s} {'instanced':>30s} {'flat':>30s} {'instanced / flat':>17s}",
             f"{'frame, ms':34s} {spread(inst['frame_ms']):>30s} {spread(flat['frame_ms']):>30s} "
             f"{ratio(inst['frame_ms'], flat['frame_ms']):17.2f}",
             f"{'moved copies, ms':34s} {spread(inst['move_ms']):>30s} {spread(flat['move_ms']):>30s} "
             f"{ratio(inst['move_ms'], flat['move_ms']):17.4f}",
             f"{'hierarchy + leaf records, bytes':34s} {inst['hierarchy_bytes']:30d} {flat['hierarchy_bytes']:30d} "
             f"{inst['hierarchy_bytes'] / flat['hierarchy_bytes']:17.4f}",
             f"{'all scene tables, bytes':34s} {inst['scene_bytes']:30d} {flat['scene_bytes']:30d} "
             f"{inst['scene_bytes'] / flat['scene_bytes']:17.4f}",
             f"{'rays of the last frame (p, s)':34s} {str(inst['rays']):>30s} {str(flat['rays']):>30s}",
             f"{'film mean per frame':34s} {inst['film_mean']:30.5f} {flat['film_mean']:30.5f}",
             f"moved copies: set_transforms (instanced, status {inst['move_status']}) against update_geometry_device on the scene's own "
             f"vertex and normal tables (flat, status {flat['move_status']}: face normals, lights, refit, LDS images, shading records)",
             f"instanced: {inst['options']}, {inst['kernel']}",
             f"flat:      {flat['options']}, {flat['kernel']}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        mode = "a" if Path(a.output).exists() else "w"
        with open(a.output, mode) as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
