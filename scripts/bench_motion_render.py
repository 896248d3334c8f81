#!/usr/bin/env python
"""A forest of moving copies through the path tracer, beside the same forest frozen at its first placements.

usage: python scripts/bench_motion_render.py [--object plant/1] [--instances 64] -o profiles/gpu_motion_render.txt

Scene: DESIGN 12's forest (scripts/bench_instanced_render.py: forest) with DESIGN 15's second placements for the plants
(scripts/bench_motion_instances.py: second_placements); the ground and the emissive quad keep one placement (lights stay static).
Moving: render.Renderer(motion=...) at shutter (0, 1); static: render.Renderer(instances=...) at M0, in the same process, one after
the other.  Reported: the frame and the move (set_motion_transforms / set_transforms).  HIP events, ms, median [min, max] of 20 after
3 warm-ups.  The measurement is a child process under its own time limit.
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

from bench_instanced_render import HEIGHT, MAXLEN, SPP, WIDTH, forest               # noqa: E402
from bench_instances import REPS, WARMUP, object_mesh, spread, timed                 # noqa: E402
from bench_motion_instances import second_placements                                 # noqa: E402

LIMIT = 900                                                                          # seconds for the measuring child


def measure(a):
    import torch
    from rodent_amd import instances as I, render as R
    objects, t0, ids, cam = forest(a)
    t1 = t0.copy()
    t1[:a.instances] = second_placements(object_mesh(a.object)[0], t0[:a.instances])
    scene = I.concat_scenes(objects)
    stream = torch.cuda.current_stream()
    d0, d1 = torch.from_numpy(t0).cuda(), torch.from_numpy(t1).cuda()
    out = {"object_tris": objects[0].num_tris, "instances": len(ids)}
    for name in ("static", "moving"):
        if name == "static":
            r = R.Renderer(scene, WIDTH, HEIGHT, SPP, MAXLEN, instances=(scene.ranges, t0, ids))
            move = lambda: r.set_transforms(d0, check=False)
        else:
            r = R.Renderer(scene, WIDTH, HEIGHT, SPP, MAXLEN, motion=(scene.ranges, t0, t1, ids), shutter=(0.0, 1.0))
            move = lambda: r.set_motion_transforms(d0, d1, check=False)
        frame = [0]
        def one_frame():
            r.render_rows(cam, frame[0], 0, HEIGHT); frame[0] += 1
        c = {"tlas_nodes": int(r.transforms_status()[1][0]), "frame_ms": timed(one_frame, stream)}
        counters = r.counters()
        c["rays"] = [int(counters["primary_rays"]), int(counters["shadow_rays"])]
        c["options"] = r.options_in_effect(); c["kernel"] = r.trace_kernel_name()
        c["film_mean"] = float(r.film().mean() / (WARMUP + REPS))
        c["move_ms"] = timed(move, stream)
        c["move_status"] = r.transforms_status()[0]
        r.close()
        out[name] = c
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--object", default="plant/1", help="scenes.py's generated kind / detail (plant/1, crown/1)")
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--measure", action="store_true", help="(internal) measure in this process and print the figures as JSON")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if a.measure:
        print("RESULT " + json.dumps(measure(a)))
        return 0
    try:
        p = subprocess.run([sys.executable, __file__, "--object", a.object, "--instances", str(a.instances), "--measure"],
                           capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"no result within {LIMIT} s", file=sys.stderr)
        return 1
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(p.stdout + p.stderr, file=sys.stderr)
        print(f"the measurement failed (exit status {p.returncode})", file=sys.stderr)
        return 1
    r = json.loads(line[0][7:])
    st, mv = r["static"], r["moving"]
    ratio = lambda x, y: np.median(x) / np.median(y)
    lines = [f"# scripts/bench_motion_render.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of "
             f"{REPS} after {WARMUP} warm-ups; {WIDTH} x {HEIGHT}, {SPP} spp, path length <= {MAXLEN}, shutter (0, 1).",
             f"scene: {r['object_tris']} triangles x {a.instances} placements with a second placement each + ground + light, "
             f"{r['instances']} instances (TLAS: {st['tlas_nodes']} nodes static, {mv['tlas_nodes']} moving)",
             f"{'':34s} {'static at M0':>30s} {'moving':>30s} {'moving / static':>17s}",
             f"{'frame, ms':34s} {spread(st['frame_ms']):>30s} {spread(mv['frame_ms']):>30s} {ratio(mv['frame_ms'], st['frame_ms']):17.2f}",
             f"{'moved copies, ms':34s} {spread(st['move_ms']):>30s} {spread(mv['move_ms']):>30s} {ratio(mv['move_ms'], st['move_ms']):17.2f}",
             f"{'rays of the last frame (p, s)':34s} {str(st['rays']):>30s} {str(mv['rays']):>30s}",
             f"{'film mean per frame':34s} {st['film_mean']:30.5f} {mv['film_mean']:30.5f}",
             f"moved copies: set_transforms (status {st['move_status']}) / set_motion_transforms (status {mv['move_status']})",
             f"static: {st['options']}, {st['kernel']}",
             f"moving: {mv['options']}, {mv['kernel']}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
