#!/usr/bin/env python
"""What deforming objects under moving instances cost against the same instances over rigid objects.

usage: python scripts/bench_motion_objects.py [--object plant/1] [--instances 64] -o profiles/gpu_motion_objects.txt

Scene: the forest of scripts/bench_motion_instances.py (N seeded instances of one generated object, each with a second placement).  The
object's key 1 is its key 0 swaying: every vertex pushed along x and z by up to 3 % of the object's diameter, growing with its height.
Rays: that script's 1 Mi camera rays and 1 Mi random segments, every ray with a seeded uniform time in [0, 1).  Reported:
build_motion_objects(out=) beside two refit_objects of the same object, and both ray sets through k_instanced_motion_objects with
key 0 -> key 1, through the same kernel with equal keys, and through k_instanced_motion over the static key-0 object under the same
placements, in one process.  HIP events, median [min, max] of 20 after 3 warm-ups.  Each step is a child process under its own time
limit; the first failure ends the run.
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
from bench_motion_instances import second_placements                                               # noqa: E402
from rodent_amd import formats as F             # noqa: E402

STEPS = (("build", 300), ("trace", 900))        # name, time limit in seconds


def second_key(v):
    """Key 1: a sway along x and z of up to 3 % of the object's diameter, growing with the square of the height."""
    lo, hi = v[:, :3].min(0), v[:, :3].max(0)
    size = float(np.linalg.norm(hi - lo))
    h = ((v[:, 1] - lo[1]) / max(float(hi[1] - lo[1]), 1e-6)).astype(np.float64)
    out = v.copy()
    out[:, 0] = (v[:, 0] + 0.03 * size * h * h * np.sin(2.0 + 3.0 * h)).astype(np.float32)
    out[:, 2] = (v[:, 2] + 0.03 * size * h * h * np.cos(1.0 + 2.0 * h)).astype(np.float32)
    return out


def step(name, a):
    import torch
    from rodent_amd import abi, gpubuild, instances
    v, ix = object_mesh(a.object)
    v1 = second_key(v)
    t0 = layout(v, a.instances)
    t1 = second_placements(v, t0)
    stream = torch.cuda.current_stream()
    out = {"object_tris": len(ix), "instances": a.instances}
    objects = instances.pack_objects([gpubuild.build_bvh2(v, ix, max_leaf=2)])
    rows = np.array([[0, len(ix)]], np.int32)
    plan = instances.plan_refit(objects, [0], rows)
    v_dev, v1_dev, ix_dev = (gpubuild._columns4(x, t, 0) for x, t in ((v, torch.float32), (v1, torch.float32), (ix, torch.int32)))
    moving = instances.build_motion_objects(objects, v_dev, v1_dev, ix_dev, plan)
    out["object_nodes"] = objects.num_nodes
    if name == "build":
        out["build_ms"] = timed(lambda: instances.build_motion_objects(objects, v_dev, v1_dev, ix_dev, plan, out=moving, check=False), stream)
        scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device="cuda")

        def two_refits():
            instances.refit_objects(objects, None, v1_dev, ix_dev, plan, scratch=scratch, check=False)
            instances.refit_objects(objects, None, v_dev, ix_dev, plan, scratch=scratch, check=False)
        out["two_refits_ms"] = timed(two_refits, stream)
        return out
    still = instances.build_motion_objects(objects, v_dev, v_dev, ix_dev, plan)
    ids = torch.zeros(a.instances, dtype=torch.int32, device="cuda")
    t0_dev, t1_dev = torch.from_numpy(t0).cuda(), torch.from_numpy(t1).cuda()
    tlas = {"moving": instances.build_motion_tlas(moving, t0_dev, t1_dev, ids, max_leaf=1),
            "still": instances.build_motion_tlas(still, t0_dev, t1_dev, ids, max_leaf=1),
            "rigid": instances.build_motion_tlas(objects, t0_dev, t1_dev, ids, max_leaf=1)}
    sets = {"moving": moving, "still": still, "rigid": objects}
    for which, t in tlas.items():
        out[f"{which}_nodes"], out[f"{which}_depth"] = t.num_nodes, t.depth
    for kind, rays in ray_sets(baked(v, ix, t0)[0]).items():
        rays_dev = abi.to_device(rays)
        times_dev = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 1.0, len(rays)).astype(np.float32)).cuda()
        hits_dev = torch.zeros(len(rays) * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        for which in ("moving", "still", "rigid"):
            trace = lambda: instances.trace_motion_async(sets[which], tlas[which], rays_dev, times_dev, hits_dev, None, len(rays))
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
    build, trace = r["build"], r["trace"]
    mrays = lambda ms: (1 << 20) / np.median(ms) / 1e3
    lines = [f"# scripts/bench_motion_objects.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of "
             f"{REPS} after {WARMUP} warm-ups; 1 Mi rays per launch, closest hit, seeded uniform times in [0, 1).",
             f"object: {build['object_tris']} triangles, {build['object_nodes']} nodes, two keys, x {build['instances']} instances, each "
             f"with a second placement",
             f"build_motion_objects(out=) {spread(build['build_ms'])} ms; two refit_objects of the same object "
             f"{spread(build['two_refits_ms'])} ms; ratio {np.median(build['build_ms']) / np.median(build['two_refits_ms']):.2f}",
             "motion TLAS nodes / depth: " + ", ".join(f"{w} {trace[w + '_nodes']} / {trace[w + '_depth']}" for w in ("moving", "still", "rigid")),
             "moving: k_instanced_motion_objects, key 0 -> key 1; still: the same kernel, equal keys; rigid: k_instanced_motion over the "
             "static key-0 object",
             f"{'rays':9s} {'moving ms':>28s} {'Mrays/s':>8s} {'still ms':>28s} {'Mrays/s':>8s} {'rigid ms':>28s} {'Mrays/s':>8s} "
             f"{'still/rigid':>11s} {'moving/rigid':>12s} {'hit share (moving, still, rigid)':>33s}"]
    for kind in ("camera", "segments"):
        m, s, g = (trace[f"{kind}_{w}_ms"] for w in ("moving", "still", "rigid"))
        lines.append(f"{kind:9s} {spread(m):>28s} {mrays(m):8.1f} {spread(s):>28s} {mrays(s):8.1f} {spread(g):>28s} {mrays(g):8.1f} "
                     f"{np.median(s) / np.median(g):11.2f} {np.median(m) / np.median(g):12.2f} "
                     + " ".join(f"{trace[kind + '_' + w + '_hit_share']:10.4f}" for w in ("moving", "still", "rigid")))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
