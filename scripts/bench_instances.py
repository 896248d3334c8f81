#!/usr/bin/env python
"""What instancing costs and saves against the same geometry baked flat.

usage: python scripts/bench_instances.py [--object plant/1] [--instances 64] -o profiles/gpu_instances.txt

Scene: N seeded instances (a rotation about y, a uniform scale in [0.7, 1.3], a grid place with jitter) of ONE generated object (scenes.py's
plant or crown at its smallest setting), its BVH2 built by gpubuild.build_bvh2.  Rays: 1 Mi camera rays over the whole layout and 1 Mi
random segments inside its bounds.  Reported: the TLAS build, instanced Mrays/s (closest hit), and as the yardstick the same triangles
baked into one mesh, built by gpubuild.build_bvh2 and traced by the default BVH2 kernel; the device bytes of both.  HIP events, median
[min, max] of 20 after 3 warm-ups.  Each step is a child process under its own time limit; the first failure ends the run.
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from rodent_amd import formats as F, raygen, scenes             # noqa: E402

WARMUP, REPS = 3, 20
STEPS = (("tlas", 300), ("instanced", 300), ("flat", 600))      # name, time limit in seconds


def spread(times):
    return f"{np.median(times):8.3f} [{min(times):8.3f}, {max(times):8.3f}]"


def object_mesh(name):
    """(vertices (3t, 4), indices (t, 4)) of the generated object: the corners of its Tri1 records."""
    _, tris = F.read_bvh(scenes.scene_bvh(name), F.BVH2_TRI1)
    _, first = np.unique(tris["prim_id"] & 0x7FFFFFFF, return_index=True)        # a spatial split repeats a triangle
    tris = tris[first]
    v = np.zeros((len(tris), 3, 4), np.float32)
    v[:, 0, :3], v[:, 1, :3], v[:, 2, :3] = tris["v0"], tris["v0"] - tris["e1"], tris["v0"] + tris["e2"]
    ix = np.zeros((len(tris), 4), np.int32)
    ix[:, :3] = np.arange(3 * len(tris)).reshape(-1, 3)
    return v.reshape(-1, 4), ix


def layout(v, n, seed=1):
    """n seeded placements (n, 12) on a square grid whose cells are 1.2 object diameters wide."""
    rng = np.random.default_rng(seed)
    lo, hi = v[:, :3].min(0), v[:, :3].max(0)
    cell = 1.2 * float(np.linalg.norm((hi - lo)[[0, 2]]))
    side = int(np.ceil(np.sqrt(n)))
    angle, scale = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.7, 1.3, n)
    t = np.zeros((n, 3, 4))
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    t[:, 0, 0], t[:, 0, 2], t[:, 1, 1], t[:, 2, 0], t[:, 2, 2] = c, s, scale, -s, c
    k = np.arange(n)
    t[:, 0, 3] = (k % side + rng.uniform(-0.1, 0.1, n)) * cell
    t[:, 2, 3] = (k // side + rng.uniform(-0.1, 0.1, n)) * cell
    return t.reshape(n, 12).astype(np.float32)


def baked(v, ix, transforms):
    """The flat scene: every instance's triangles in world space."""
    n, m = len(transforms), transforms.reshape(-1, 3, 4).astype(np.float64)
    world = np.zeros((n, len(v), 4), np.float32)
    world[:, :, :3] = np.einsum("nij,vj->nvi", m[:, :, :3], v[:, :3].astype(np.float64)) + m[:, None, :, 3]
    index = np.tile(ix, (n, 1, 1))
    index[:, :, :3] += (np.arange(n) * len(v))[:, None, None]
    return world.reshape(-1, 4), index.reshape(-1, 4).astype(np.int32)


def ray_sets(world):
    lo, hi = world[:, :3].min(0), world[:, :3].max(0)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    eye = centre + np.float32([0.0, 0.45, 0.75]) * size
    return {"camera": raygen.primary_rays(eye, centre - eye, (0, 1, 0), 55.0, 1024, 1024, 0.0, 1e9),
            "segments": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, 1.0)}


def timed(fn, stream):
    import torch
    times = []
    for _ in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times[WARMUP:]


def step(name, a):
    import torch
    from rodent_amd import abi, gpubuild, instances
    v, ix = object_mesh(a.object)
    transforms = layout(v, a.instances)
    stream = torch.cuda.current_stream()
    out = {"object_tris": len(ix), "instances": a.instances}
    if name == "flat":
        world, index = baked(v, ix, transforms)
        w_dev, i_dev = torch.from_numpy(world).cuda(), torch.from_numpy(index).cuda()      # uploaded once: the clock sees no copy
        bvh = gpubuild.build_bvh2(w_dev, i_dev, max_leaf=2)
        out["flat_bytes"] = bvh.num_nodes * F.NODE2.itemsize + bvh.num_tris * F.TRI1.itemsize
        out["flat_build_ms"] = timed(lambda: gpubuild.build_bvh2(w_dev, i_dev, max_leaf=2, scratch=bvh.scratch, out=bvh), stream)
        trace = lambda rays, hits: abi.traverse_async(bvh, rays, hits, 1 << 20)
    else:
        obj = gpubuild.build_bvh2(v, ix, max_leaf=2)
        objects = instances.pack_objects([obj])
        ids = torch.zeros(a.instances, dtype=torch.int32, device="cuda")               # transforms and ids live on the device
        t_dev = torch.from_numpy(transforms).cuda()
        tlas = instances.build_tlas(objects, t_dev, ids, max_leaf=1)
        out["instanced_bytes"] = objects.device_bytes + tlas.device_bytes
        out["tlas_nodes"], out["tlas_depth"] = tlas.num_nodes, tlas.depth
        if name == "tlas":
            out["tlas_build_ms"] = timed(lambda: instances.build_tlas(objects, t_dev, ids, max_leaf=1, out=tlas), stream)
            return out
        trace = lambda rays, hits: instances.trace_async(objects, tlas, rays, hits, None, 1 << 20)
        world = baked(v, ix, transforms)[0]
    for kind, rays in ray_sets(world).items():
        rays_dev = abi.to_device(rays)
        hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        out[f"{kind}_ms"] = timed(lambda: trace(rays_dev, hits_dev), stream)
        abi.check_errors(0)
        out[f"{kind}_hit_share"] = float((abi.from_device(hits_dev, F.HIT1)["tri_id"] >= 0).mean())
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
    tlas, inst, flat = r["tlas"], r["instanced"], r["flat"]
    mrays = lambda ms: (1 << 20) / np.median(ms) / 1e3
    lines = [f"# scripts/bench_instances.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of {REPS} "
             f"after {WARMUP} warm-ups; 1 Mi rays per launch, closest hit.",
             f"object: {tlas['object_tris']} triangles x {tlas['instances']} instances = {tlas['object_tris'] * tlas['instances']}",
             f"TLAS: {tlas['tlas_nodes']} nodes, depth {tlas['tlas_depth']}; build (instances.build_tlas(out=tlas) on device tensors: the "
             f"descriptors' assembly, rodent_hip_build_tlas, the info words' copy) "
             f"{spread(tlas['tlas_build_ms'])} ms",
             f"flat rebuild (gpubuild.build_bvh2 on device tensors, max_leaf 2, with its info words' copy): {spread(flat['flat_build_ms'])} ms",
             f"device bytes: instanced {inst['instanced_bytes']}, flat {flat['flat_bytes']} "
             f"({flat['flat_bytes'] / inst['instanced_bytes']:.1f} x)",
             f"{'rays':9s} {'instanced ms':>28s} {'Mrays/s':>8s} {'flat ms':>28s} {'Mrays/s':>8s} {'instanced/flat':>14s} "
             f"{'hit share (both)':>17s}"]
    for kind in ("camera", "segments"):
        i_ms, f_ms = inst[f"{kind}_ms"], flat[f"{kind}_ms"]
        lines.append(f"{kind:9s} {spread(i_ms):>28s} {mrays(i_ms):8.1f} {spread(f_ms):>28s} {mrays(f_ms):8.1f} "
                     f"{np.median(i_ms) / np.median(f_ms):14.2f} {inst[kind + '_hit_share']:8.4f} {flat[kind + '_hit_share']:8.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
