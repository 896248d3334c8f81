#!/usr/bin/env python
"""What one geometry update of a loaded scene costs through each path.

usage: python scripts/bench_scene_update.py --scenes cornell atrium -o profiles/gpu_scene_refit_device.txt

Per scene, on a renderer with a device-built hierarchy (max_leaf 2), K = 20 updates after 3 warm-ups through
  * the host path, Renderer.update_geometry (rodent_hip_scene_refit): the baseline.  Its tables (vertices, normals, face normals, lights)
    come from tests/scene_update_model.py and are computed BEFORE the clock starts -- a caller's own CPU code would be faster than numpy,
    so only the call is timed; what the model took is reported beside it, uncounted;
  * the device path, Renderer.update_geometry_device, fed by a torch shear of the vertex tensor (the shear's two launches are inside
    the clock).
Wall time is taken around the call plus a device synchronisation: median [min, max].  For the device path the device-event time of the
enqueued launches alone is given too.  Both paths move the scene by the same shear, alternating between two amounts; after the last
update the two renderers' tables are compared byte for byte.
"""
import argparse
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import scene_update_model as M                                       # noqa: E402
from rodent_amd import render as Rn, scene as S, scenes             # noqa: E402

WARMUP, REPS = 3, 20
SHEARS = ((0.25, 0.1), (-0.15, 0.3))


def spread(times):
    return f"{np.median(times):9.3f} [{min(times):8.3f}, {max(times):8.3f}]"


def tables(r):
    out = r.scene_tables()
    out["nodes"], out["tris"] = r.scene_bvh()
    return {k: v.tobytes() for k, v in out.items() if v is not None}


def bench_scene(name, workdir):
    import copy
    import torch
    obj = ROOT / "tests" / "golden" / "cornell_box.obj" if name == "cornell" else scenes.scene_obj(name)
    scene = S.convert(obj, Path(workdir) / f"{name}.rscene")
    # the host path's tables, from the model
    t0 = time.perf_counter()
    moved = []
    for kx, kz in SHEARS:
        m = copy.copy(scene)
        m.vertices = M.shear(scene.vertices, kx, kz)
        m.face_normals = M.face_normals(m.vertices, scene.indices)
        m.normals = M.smooth_normals(m.face_normals, scene.indices, len(m.vertices))
        m.lights = M.light_records(scene.lights, m.vertices, scene.indices, scene.materials, scene.light_ids)
        moved.append(m)
    model_ms = (time.perf_counter() - t0) * 1e3 / len(SHEARS)
    r = Rn.Renderer(scene, 64, 64, 1, 4, gpu_bvh=2)
    try:
        host = []
        for i in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.update_geometry(moved[i % 2])
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        host_tables = tables(r)
        nodes = len(r.scene_bvh()[0])
    finally:
        r.close()
    r = Rn.Renderer(scene, 64, 64, 1, 4, gpu_bvh=2)
    try:
        r.prepare_update()
        base = torch.from_numpy(scene.vertices).cuda()
        stream = torch.cuda.current_stream()
        wall, events = [], []
        for i in range(WARMUP + REPS):
            kx, kz = SHEARS[i % 2]
            first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = base.clone()
            v[:, 0] = base[:, 0] + float(np.float32(kx)) * base[:, 1]
            v[:, 2] = base[:, 2] + float(np.float32(kz)) * base[:, 1]
            first.record(stream)
            r.update_geometry_device(v, check=False)
            last.record(stream)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            events.append(first.elapsed_time(last))
        flags = r.update_status()[0]
        same = tables(r) == host_tables
    finally:
        r.close()
    ratio = np.median(host[WARMUP:]) / np.median(wall[WARMUP:])
    return (f"{name:8s} {scene.num_tris:8d} {nodes:8d}  {spread(host[WARMUP:])}  {spread(wall[WARMUP:])}  {spread(events[WARMUP:])}  "
            f"{ratio:7.1f}  {model_ms:9.1f}  {'yes' if same and not flags else 'NO'}")


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", nargs="+", default=["cornell", "atrium"])
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    lines = [f"# scripts/bench_scene_update.py on {torch.cuda.get_device_name(0)}; ms per update, median [min, max] of {REPS} after "
             f"{WARMUP} warm-ups.  host: wall time of Renderer.update_geometry + a device synchronisation, its tables computed beforehand "
             "(model ms: what tests/scene_update_model.py took for them, not counted).  device: wall time of a torch shear + "
             "Renderer.update_geometry_device + a device synchronisation; events: device-event time of what the call enqueued.  "
             "host/device: ratio of the wall medians.  same: both renderers' tables and hierarchy equal byte for byte after the last "
             "update.",
             f"{'scene':8s} {'tris':>8s} {'nodes':>8s}  {'host wall ms':>30s}  {'device wall ms':>30s}  {'device events ms':>30s}  "
             f"{'host/device':>7s}  {'model ms':>9s}  same"]
    with tempfile.TemporaryDirectory() as d:
        for name in a.scenes:
            lines.append(bench_scene(name, d))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(text)


if __name__ == "__main__":
    main()
