#!/usr/bin/env python
"""What a time per ray over moving instances costs against the same instances frozen at time 0.

usage: python scripts/bench_motion_instances.py [--object plant/1] [--instances 64] -o profiles/gpu_motion_instances.txt

Scene: the forest of scripts/bench_instances.py (N seeded instances of one generated object); every copy gets a second placement, its
first turned by a seeded angle of up to 0.1 rad about y and shifted by up to 5 % of the object's diameter.  Rays: that script's 1 Mi
camera rays and 1 Mi random segments, every ray with a seeded uniform time in [0, 1).  Reported: build_motion_tlas beside build_tlas,
and both ray sets through k_instanced_motion beside the same rays through k_instanced at M0, in the same process.  HIP events, median
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
sys.path.insert(0, str(ROOT / "scripts"))

from bench_instances import REPS, WARMUP, baked, layout, object_mesh, ray_sets, spread, timed      # noqa: E402
from rodent_amd import formats as F             # noqa: E402

STEPS = (("tlas", 300), ("trace", 600))         # name, time limit in seconds


def second_placements(v, transforms, seed=2):
    """Every placement turned by a seeded angle in [-0.1, 0.1] rad about y (about the copy's own origin) and shifted by up to 5 % of
    the object's diameter."""
    rng = np.random.default_rng(seed)
    n = len(transforms)
    size = float(np.linalg.norm(v[:, :3].max(0) - v[:, :3].min(0)))
    angle = rng.uniform(-0.1, 0.1, n)
    turn = np.zeros((n, 3, 3))
    turn[:, 0, 0], turn[:, 0, 2], turn[:, 1, 1], turn[:, 2, 0], turn[:, 2, 2] = np.cos(angle), np.sin(angle), 1.0, -np.sin(angle), np.cos(angle)
    t = transforms.reshape(n, 3, 4).astype(np.float64)
    out = t.copy()
    out[:, :, :3] = turn @ t[:, :, :3]
    out[:, :, 3] += rng.uniform(-0.05, 0.05, (n, 3)) * size
    return out.reshape(n, 12).astype(np.float32)


def step(name, a):
    import torch
    from rodent_amd import abi, gpubuild, instances
    v, ix = object_mesh(a.object)
    t0 = layout(v, a.instances)
    t1 = second_placements(v, t0)
    stream = torch.cuda.current_stream()
    out = {"object_tris": len(ix), "instances": a.instances}
    objects = instances.pack_objects([gpubuild.build_bvh2(v, ix, max_leaf=2)])
    ids = torch.zeros(a.instances, dtype=torch.int32, device="cuda")                   # transforms and ids live on the device
    t0_dev, t1_dev = torch.from_numpy(t0).cuda(), torch.from_numpy(t1).cuda()
    static = instances.build_tlas(objects, t0_dev, ids, max_leaf=1)
    motion = instances.build_motion_tlas(objects, t0_dev, t1_dev, ids, max_leaf=1)
    out["static_nodes"], out["static_depth"], out["motion_nodes"], out["motion_depth"] = (static.num_nodes, static.depth, motion.num_nodes,
                                                                                          motion.depth)
    if name == "tlas":
        out["static_build_ms"] = timed(lambda: instances.build_tlas(objects, t0_dev, ids, max_leaf=1, out=static), stream)
        out["motion_build_ms"] = timed(lambda: instances.build_motion_tlas(objects, t0_dev, t1_dev, ids, max_leaf=1, out=motion), stream)
        return out
    for kind, rays in ray_sets(baked(v, ix, t0)[0]).items():
        rays_dev = abi.to_device(rays)
        times_dev = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 1.0, len(rays)).astype(np.float32)).cuda()
        hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        for which, trace in (("static", lambda: instances.trace_async(objects, static, rays_dev, hits_dev, None, len(rays))),
                             ("motion", lambda: instances.trace_motion_async(objects, motion, rays_dev, times_dev, hits_dev, None,
                                                                             len(rays)))):
            out[f"{kind}_{which}_ms"] = timed(trace, stream)
            abi.check_errors(0)
            out[f"{kind}_{which}_hit_share"] = float((abi.from_device(hits_dev, F.HIT1)["tri_id"] >= 0).mean())
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
    tlas, trace = r["tlas"], r["trace"]
    mrays = lambda ms: (1 << 20) / np.median(ms) / 1e3
    lines = [f"# scripts/bench_motion_instances.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of "
             f"{REPS} after {WARMUP} warm-ups; 1 Mi rays per launch, closest hit, seeded uniform times in [0, 1).",
             f"object: {tlas['object_tris']} triangles x {tlas['instances']} instances, each with a second placement",
             f"static TLAS at M0: {tlas['static_nodes']} nodes, depth {tlas['static_depth']}; build_tlas(out=) {spread(tlas['static_build_ms'])} ms",
             f"motion TLAS:       {tlas['motion_nodes']} nodes, depth {tlas['motion_depth']}; build_motion_tlas(out=) "
             f"{spread(tlas['motion_build_ms'])} ms",
             f"{'rays':9s} {'k_instanced at M0 ms':>28s} {'Mrays/s':>8s} {'k_instanced_motion ms':>28s} {'Mrays/s':>8s} {'motion/static':>14s} "
             f"{'hit share (static, motion)':>27s}"]
    for kind in ("camera", "segments"):
        s_ms, m_ms = trace[f"{kind}_static_ms"], trace[f"{kind}_motion_ms"]
        lines.append(f"{kind:9s} {spread(s_ms):>28s} {mrays(s_ms):8.1f} {spread(m_ms):>28s} {mrays(m_ms):8.1f} "
                     f"{np.median(m_ms) / np.median(s_ms):14.2f} {trace[kind + '_static_hit_share']:13.4f} "
                     f"{trace[kind + '_motion_hit_share']:13.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
