#!/usr/bin/env python
"""What a frame of a deforming mesh costs, beside the same mesh standing still through three other routes.

usage: python scripts/bench_deforming_render.py [--scene atrium] -o profiles/gpu_deforming_render.txt

Scene: DESIGN 17's -- the atrium, key 1 = key 0 under tests/refit_model.py's deform (seed 1), except that the corners of emissive
triangles keep key 0's rows (lights stay static) -- at 1024 x 576, 4 spp, paths of at most 8.  One process, one renderer after the
other; HIP events, ms, median [min, max] of 20 after 3 warm-ups:
  (a) render.Renderer(deform=...) at shutter (0, 1);
  (b) the same renderer with both keys equal to key 0: the price of the records and the interpolation alone;
  (c) render.Renderer(motion=...) over one identity instance of the key-0 mesh: the same schedule (one chunk per one-wave workgroup, the
      whole stack in LDS), static records;
  (d) the flat render.Renderer(gpu_bvh=2) at key 0: the production kernels;
and the update: set_motion_keys (both keys, smooth normals recomputed) beside update_geometry_device (one key, smooth normals).
The measurement is a child process under its own time limit.
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
sys.path.insert(0, str(ROOT / "tests"))

from bench_instances import REPS, WARMUP, spread, timed                              # noqa: E402

WIDTH, HEIGHT, SPP, MAXLEN = 1024, 576, 4, 8
LIMIT = 900                                                                          # seconds for the measuring child
IDENTITY = np.float32([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]])


def measure(a):
    import torch
    import refit_model
    from rodent_amd import build, instances as I, render as R, scenes
    from rodent_amd import scene as S
    scenes.DATA.mkdir(parents=True, exist_ok=True)
    rs = scenes.DATA / f"{a.scene.replace('/', '-')}.rscene"
    subprocess.run([str(build.BIN_DIR / "converter"), str(scenes.scene_obj(a.scene)), "-o", str(rs)], check=True, stdout=subprocess.DEVNULL)
    sc = S.Scene(rs)
    eye, d, up, fov = scenes.CAMERAS[a.scene.split("/")[0]]
    cam = S.camera_settings(eye, d, up, fov, WIDTH, HEIGHT)
    v0 = np.ascontiguousarray(sc.vertices, np.float32)
    v1 = refit_model.deform(sc.vertices, sc.indices, seed=1).astype(np.float32)
    ix = np.asarray(sc.indices).reshape(-1, 4)
    lit = np.unique(ix[np.asarray(sc.materials)["emissive"][ix[:, 3]] != 0, :3])
    v1[lit] = v0[lit]
    n1 = R.smooth_normals(v1, ix)
    stream = torch.cuda.current_stream()
    d0, d1 = torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()
    out = {"tris": int(sc.num_tris), "vertices": len(v0), "emitter_corners": int(len(lit))}

    def frames(r, name):
        frame = [0]

        def one_frame():
            r.render_rows(cam, frame[0], 0, HEIGHT); frame[0] += 1
        c = {"frame_ms": timed(one_frame, stream)}
        counters = r.counters()
        c["rays"] = [int(counters["primary_rays"]), int(counters["shadow_rays"])]
        c["options"] = r.options_in_effect(); c["kernel"] = r.trace_kernel_name()
        c["film_mean"] = float(r.film().mean() / (WARMUP + REPS))
        out[name] = c
        return c
    r = R.Renderer(sc, WIDTH, HEIGHT, SPP, MAXLEN, deform=(v1, n1), shutter=(0.0, 1.0))
    out["nodes"] = int(r.motion_keys_status()[1][0])
    c = frames(r, "deforming")
    c["update_ms"] = timed(lambda: r.set_motion_keys(d0, d1, check=False), stream)
    c["update_status"] = r.motion_keys_status()[0]
    r.set_motion_keys(d0, d0, torch.from_numpy(np.ascontiguousarray(sc.normals)).cuda(), torch.from_numpy(np.ascontiguousarray(sc.normals)).cuda())
    r.clear()
    frames(r, "equal_keys")
    r.close()
    one = I.concat_scenes([sc])
    r = R.Renderer(one, WIDTH, HEIGHT, SPP, MAXLEN, motion=(one.ranges, IDENTITY, IDENTITY, [0]), shutter=(0.0, 1.0))
    frames(r, "one_instance")
    r.close()
    r = R.Renderer(sc, WIDTH, HEIGHT, SPP, MAXLEN, gpu_bvh=2)
    c = frames(r, "flat")
    r.prepare_update(True)
    c["update_ms"] = timed(lambda: r.update_geometry_device(d1, check=False), stream)
    c["update_status"] = r.update_status()[0]
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--measure", action="store_true", help="(internal) measure in this process and print the figures as JSON")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if a.measure:
        print("RESULT " + json.dumps(measure(a)))
        return 0
    try:
        p = subprocess.run([sys.executable, __file__, "--scene", a.scene, "--measure"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"no result within {LIMIT} s", file=sys.stderr)
        return 1
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(p.stdout + p.stderr, file=sys.stderr)
        print(f"the measurement failed (exit status {p.returncode})", file=sys.stderr)
        return 1
    r = json.loads(line[0][7:])
    rows = (("(a) deform=, shutter (0, 1)", "deforming"), ("(b) deform=, key 1 = key 0", "equal_keys"),
            ("(c) motion=, 1 identity instance", "one_instance"), ("(d) gpu_bvh=2 at key 0", "flat"))
    base = np.median(r["deforming"]["frame_ms"])
    lines = [f"# scripts/bench_deforming_render.py --scene {a.scene}; HIP events, ms, median [min, max] of {REPS} after {WARMUP} warm-ups; "
             f"{WIDTH} x {HEIGHT}, {SPP} spp, path length <= {MAXLEN}; key 1 = refit_model.deform(seed 1), emitters' corners kept.",
             f"{a.scene}: {r['tris']} triangles, {r['vertices']} vertices ({r['emitter_corners']} of them corners of emitters), "
             f"{r['nodes']} nodes (max_leaf 2)",
             f"{'frame':34s} {'ms':>30s} {'(a) / it':>9s} {'rays of the last frame (p, s)':>32s} {'film mean':>10s}"]
    for label, name in rows:
        c = r[name]
        lines.append(f"{label:34s} {spread(c['frame_ms']):>30s} {base / np.median(c['frame_ms']):9.2f} {str(c['rays']):>32s} "
                     f"{c['film_mean']:10.5f}")
    de, fl = r["deforming"], r["flat"]
    lines += [f"{'update':34s} {'ms':>30s}",
              f"{'set_motion_keys, both keys':34s} {spread(de['update_ms']):>30s}   (status {de['update_status']})",
              f"{'update_geometry_device, one key':34s} {spread(fl['update_ms']):>30s}   (status {fl['update_status']}; "
              f"{np.median(de['update_ms']) / np.median(fl['update_ms']):.2f} x)"]
    lines += [f"{label[:3]}: {r[name]['options']}, {r[name]['kernel']}" for label, name in rows]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
