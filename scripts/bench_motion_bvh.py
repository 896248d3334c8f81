#!/usr/bin/env python
"""What a time per ray over a deforming mesh costs.

usage: python scripts/bench_motion_bvh.py [--scene atrium] -o profiles/gpu_motion_bvh.txt

Scene: the atrium built with build_bvh2 (max_leaf 2); key 1 is key 0 under tests/refit_model.py's deform (seed 1).  Rays: 1 Mi camera
rays and 1 Mi random segments, every ray with a seeded uniform time in [0, 1).  Reported, HIP events, median [min, max] of 20 after 3
warm-ups:
  (a) rodent_hip_build_motion_bvh2_tri1 beside one rodent_hip_refit_bvh2_tri1 of the same tree;
  (b) k_bvh2_motion beside k_instanced over ONE identity instance of the key-0 tree: the same schedule (one chunk per one-wave
      workgroup, the whole stack in LDS), so the difference is the interpolation and the second half of every record;
  (c) k_bvh2_motion beside hip_traverse_bvh2_tri1_async on the key-0 tree: the distance to the production kernel.
Two rows more take the scene out of (b): k_bvh2_motion over records whose two keys are BOTH key 0 (the interpolation and the second
half-line are paid, the tree is the static one), and k_instanced over the tree refitted to key 1 (no interpolation, the boxes of the
deformed mesh over a topology built for key 0).
Each step is a child process under its own time limit; the first failure ends the run.
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from bench_instances import REPS, WARMUP, spread, timed      # noqa: E402
from rodent_amd import formats as F             # noqa: E402

STEPS = (("build", 300), ("trace", 600))        # name, time limit in seconds
IDENTITY = np.float32([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]])


def step(name, a):
    import torch
    import refit_model
    from rodent_amd import abi, build, gpubuild, instances, motion, raygen, scenes
    from rodent_amd import scene as S
    scenes.DATA.mkdir(parents=True, exist_ok=True)
    rs = scenes.DATA / f"{a.scene.replace('/', '-')}.rscene"
    subprocess.run([str(build.BIN_DIR / "converter"), str(scenes.scene_obj(a.scene)), "-o", str(rs)], check=True, stdout=subprocess.DEVNULL)
    sc = S.Scene(rs)
    v0 = torch.from_numpy(sc.vertices).cuda()
    v1 = torch.from_numpy(refit_model.deform(sc.vertices, sc.indices, seed=1)).cuda()
    ix = torch.from_numpy(sc.indices).cuda()
    stream = torch.cuda.current_stream()
    bvh = gpubuild.build_bvh2(v0, ix, max_leaf=2)
    mbvh = motion.build_motion_bvh2(bvh, v0, v1, ix)
    out = {"tris": int(sc.num_tris), "nodes": bvh.num_nodes, "records": bvh.num_tris,
           "static_bytes": bvh.num_nodes * F.NODE2.itemsize + bvh.num_tris * F.TRI1.itemsize,
           "motion_bytes": bvh.num_nodes * F.MOTION_NODE2.itemsize + bvh.num_tris * F.MOTION_TRI1.itemsize,
           "scratch_bytes": int(abi.lib().rodent_hip_motion_bvh2_scratch_bytes(bvh.num_nodes, bvh.num_tris))}
    if name == "build":
        l = abi.lib()
        info = torch.empty(4, dtype=torch.int32, device="cuda")
        copy = abi.DeviceBvh.from_tensors(2, bvh.nodes.clone(), bvh.tris.clone(), bvh.num_nodes, bvh.num_tris)
        refit_scratch = torch.empty(l.rodent_hip_refit_scratch_bytes(bvh.num_nodes, bvh.num_tris), dtype=torch.uint8, device="cuda")
        s = C.c_void_p(stream.cuda_stream)

        def one_refit():
            assert l.rodent_hip_refit_bvh2_tri1(0, v1.data_ptr(), v1.shape[0], ix.data_ptr(), ix.shape[0], copy.nodes.data_ptr(),
                                                copy.num_nodes, copy.tris.data_ptr(), copy.num_tris, refit_scratch.data_ptr(),
                                                info.data_ptr(), s) == 0

        def one_motion_build():
            assert l.rodent_hip_build_motion_bvh2_tri1(0, v0.data_ptr(), v1.data_ptr(), v0.shape[0], ix.data_ptr(), ix.shape[0],
                                                       bvh.nodes.data_ptr(), bvh.num_nodes, bvh.tris.data_ptr(), bvh.num_tris,
                                                       mbvh.nodes.data_ptr(), mbvh.tris.data_ptr(), mbvh.scratch.data_ptr(),
                                                       info.data_ptr(), s) == 0
        out["refit_ms"] = timed(one_refit, stream)
        assert info.cpu().numpy().tolist() == [bvh.num_nodes, bvh.num_tris, 0, 0]
        out["motion_build_ms"] = timed(one_motion_build, stream)
        assert info.cpu().numpy().tolist() == [bvh.num_nodes, bvh.num_nodes + bvh.num_tris, 0, bvh.num_nodes]
        return out
    still = motion.build_motion_bvh2(bvh, v0, v0, ix)                                  # both keys are key 0
    at_key1 = gpubuild.refit_bvh2(gpubuild.build_bvh2(v0, ix, max_leaf=2), v1, ix)       # the static tree of key 1, same topology
    objects, objects1 = instances.pack_objects([bvh]), instances.pack_objects([at_key1])
    tlas = instances.build_tlas(objects, torch.from_numpy(IDENTITY).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"), max_leaf=1)
    eye, d, up, fov = scenes.CAMERAS[a.scene.split("/")[0]]
    lo, hi = sc.vertices[:, :3].min(0), sc.vertices[:, :3].max(0)
    ray_sets = {"camera": raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX),
                "segments": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX)}
    for kind, rays in ray_sets.items():
        n = len(rays)
        rays_dev = abi.to_device(rays)
        times_dev = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 1.0, n).astype(np.float32)).cuda()
        hits_dev = torch.zeros(n * F.HIT1.itemsize, dtype=torch.uint8, device="cuda")
        for which, trace in (("production", lambda: abi.traverse_async(bvh, rays_dev, hits_dev, n)),
                             ("instanced", lambda: instances.trace_async(objects, tlas, rays_dev, hits_dev, None, n)),
                             ("instanced1", lambda: instances.trace_async(objects1, tlas, rays_dev, hits_dev, None, n)),
                             ("still", lambda: motion.trace_motion_async(still, rays_dev, times_dev, hits_dev, n)),
                             ("motion", lambda: motion.trace_motion_async(mbvh, rays_dev, times_dev, hits_dev, n))):
            out[f"{kind}_{which}_ms"] = timed(trace, stream)
            abi.check_errors(0)
            out[f"{kind}_{which}_hit_share"] = float((abi.from_device(hits_dev, F.HIT1)["tri_id"] >= 0).mean())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one step and print its figures as JSON")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a)))
        return 0
    r = {}
    for name, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, __file__, "--scene", a.scene, "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name} failed (no result within {limit} s): nothing further is run", file=sys.stderr)
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout + p.stderr, file=sys.stderr)
            print(f"step {name} failed (exit status {p.returncode}): nothing further is run", file=sys.stderr)
            return 1
        r[name] = json.loads(line[0][7:])
    b, t = r["build"], r["trace"]
    mrays = lambda ms: (1 << 20) / np.median(ms) / 1e3
    lines = [f"# scripts/bench_motion_bvh.py --scene {a.scene}; HIP events, ms, median [min, max] of {REPS} after {WARMUP} warm-ups; 1 Mi rays "
             f"per launch, closest hit, seeded uniform times in [0, 1); key 1 = refit_model.deform(seed 1).",
             f"{a.scene}: {b['tris']} triangles, build_bvh2(max_leaf 2): {b['nodes']} nodes, {b['records']} Tri1 records; static records "
             f"{b['static_bytes'] / 2 ** 20:.1f} MiB, motion records {b['motion_bytes'] / 2 ** 20:.1f} MiB, build scratch "
             f"{b['scratch_bytes'] / 2 ** 20:.1f} MiB",
             f"(a) rodent_hip_refit_bvh2_tri1 (one key)      {spread(b['refit_ms'])} ms",
             f"    rodent_hip_build_motion_bvh2_tri1         {spread(b['motion_build_ms'])} ms   "
             f"{np.median(b['motion_build_ms']) / np.median(b['refit_ms']):.2f} x one refit",
             f"{'rays':9s} {'kernel':>28s} {'ms':>28s} {'Mrays/s':>8s} {'motion / it':>12s} {'hit share':>10s}"]
    for kind in ("camera", "segments"):
        m = np.median(t[f"{kind}_motion_ms"])
        for label, which in (("(c) hip_traverse_bvh2_tri1", "production"), ("(b) k_instanced, 1 identity", "instanced"),
                             ("k_instanced, tree at key 1", "instanced1"), ("k_bvh2_motion, key 1 = key 0", "still"),
                             ("k_bvh2_motion", "motion")):
            ms = t[f"{kind}_{which}_ms"]
            lines.append(f"{kind:9s} {label:>28s} {spread(ms):>28s} {mrays(ms):8.1f} {m / np.median(ms):12.2f} "
                         f"{t[f'{kind}_{which}_hit_share']:10.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
