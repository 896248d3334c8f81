#!/usr/bin/env python
"""Geometry that deforms inside an instanced object, against the same geometry baked flat; the forest refit against per-object refits
(DESIGN.md 13).

usage: python scripts/bench_instanced_deform.py [--object plant/1] [--instances 64] -o profiles/gpu_instanced_deform.txt

Scene: scripts/bench_instanced_render.py's forest -- N placements of ONE generated plant over a ground quad, under an emissive quad.
D = {the plant}.  Measured, HIP events, ms, median [min, max] of 20 after 3 warm-ups:
  deform     Renderer.deform_objects on the scene's own vertex and normal tables against Renderer.update_geometry_device of the
             forest baked flat on ITS own tables: the launches a moving plant costs, without a copy on either side; deform_objects
             also with smooth normals, and with new matrices in the same call beside set_transforms alone;
  refit      rodent_hip_refit_objects over K = 256 packed twelve-triangle objects against a host loop of 256
             rodent_hip_refit_bvh2_tri1 calls on the same packed arrays (one stream, no wait in between), and over the one plant
             against rodent_hip_refit_bvh2_tri1 on it; both forms must leave the same bytes.
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

from bench_instanced_render import HEIGHT, MAXLEN, SPP, WIDTH, baked, forest                # noqa: E402
from bench_instances import REPS, WARMUP, object_mesh, spread, timed                         # noqa: E402
from rodent_amd import formats as F                                                        # noqa: E402

STEPS = (("deform", 600), ("flat", 900), ("refit", 600))
K_SMALL = 256
CUBE = np.int32([(0, 3, 2), (0, 2, 1), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (0, 4, 7),
                 (0, 7, 3)])


def small_objects(k):
    """(vertices, indices, rows) of k unit cubes side by side: 8 vertices and 12 triangles each, one concatenated table."""
    corner = np.float32([(-.5, -.5, -.5), (.5, -.5, -.5), (.5, .5, -.5), (-.5, .5, -.5), (-.5, -.5, .5), (.5, -.5, .5), (.5, .5, .5),
                         (-.5, .5, .5)])
    v = np.zeros((k, 8, 4), np.float32)
    v[:, :, :3] = corner[None] + np.float32([2.0, 0, 0]) * np.arange(k, dtype=np.float32)[:, None, None]
    ix = np.zeros((k, 12, 4), np.int32)
    ix[:, :, :3] = CUBE[None] + 8 * np.arange(k)[:, None, None]
    return v.reshape(-1, 4), ix.reshape(-1, 4), np.stack([12 * np.arange(k), np.full(k, 12)], 1).astype(np.int32)


def forest_against_loop(out, name, bvhs, v, ix, rows, stream):
    """Times instances.refit_objects over all packed `bvhs` against the loop of single refits on the same packed arrays."""
    import torch
    from rodent_amd import abi, instances as I
    objects = I.pack_objects(bvhs)
    plan = I.plan_refit(objects, np.arange(len(bvhs)), rows)
    vd, ixd = torch.from_numpy(v).cuda(), torch.from_numpy(ix).cuda()
    l = abi.lib()
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    raw = C.c_void_p(stream.cuda_stream)
    table = objects.table

    def forest_refit():
        rc = l.rodent_hip_refit_objects(0, vd.data_ptr(), len(v), ixd.data_ptr(), len(ix), objects.nodes.data_ptr(),
                                        objects.tris.data_ptr(), objects.table_dev.data_ptr(), len(table), plan.table_dev.data_ptr(),
                                        plan.num_listed, plan.num_nodes, plan.num_recs, scratch.data_ptr(), info.data_ptr(), raw)
        assert rc == 0, rc

    def loop():
        for o, (first, n) in zip(table, rows):
            rc = l.rodent_hip_refit_bvh2_tri1(0, vd.data_ptr(), len(v), ixd.data_ptr() + 16 * int(first), int(n),
                                              objects.nodes.data_ptr() + F.NODE2.itemsize * int(o["node_offset"]), int(o["num_nodes"]),
                                              objects.tris.data_ptr() + F.TRI1.itemsize * int(o["tri_offset"]), int(o["num_tris"]),
                                              scratch.data_ptr(), info.data_ptr(), raw)
            assert rc == 0, rc
    out[name + "_forest_ms"] = timed(forest_refit, stream)
    after_forest = objects.buffer.clone()
    words = info.cpu().tolist()
    assert words == [plan.num_nodes, plan.num_recs, 0, 0], words
    out[name + "_loop_ms"] = timed(loop, stream)
    assert torch.equal(after_forest, objects.buffer), "the loop of single refits leaves other bytes than the forest refit"
    out[name + "_nodes"], out[name + "_recs"] = plan.num_nodes, plan.num_recs


def step(name, a):
    import torch
    from rodent_amd import gpubuild, instances as I, render as R
    stream = torch.cuda.current_stream()
    out = {}
    if name == "refit":
        v, ix, rows = small_objects(K_SMALL)
        cube = gpubuild.build_bvh2(v[:8], ix[:12], max_leaf=2)
        forest_against_loop(out, "small", [cube] * K_SMALL, v, ix, rows, stream)
        v, ix = object_mesh(a.object)
        forest_against_loop(out, "plant", [gpubuild.build_bvh2(v, ix, max_leaf=2)], v, ix, np.int32([[0, len(ix)]]), stream)
        return out
    objects, transforms, ids, cam = forest(a)
    scene = I.concat_scenes(objects)
    out["object_tris"], out["instances"] = objects[0].num_tris, len(ids)
    if name == "deform":
        r = R.Renderer(scene, WIDTH, HEIGHT, SPP, MAXLEN, instances=(scene.ranges, transforms, ids))
        r.prepare_deform([0])
        tables = r.scene_table_pointers()
        out["given_ms"] = timed(lambda: r.deform_objects(tables["vertices"], tables["normals"], check=False), stream)
        out["given_status"] = r.deform_status()[0]
        out["smooth_ms"] = timed(lambda: r.deform_objects(tables["vertices"], check=False), stream)
        out["smooth_status"] = r.deform_status()[0]
        t_dev = torch.from_numpy(transforms).cuda()
        out["with_matrices_ms"] = timed(lambda: r.deform_objects(tables["vertices"], tables["normals"], t_dev, check=False), stream)
        out["move_ms"] = timed(lambda: r.set_transforms(t_dev, check=False), stream)
        out["refit_words"] = r.deform_status()[1]
    else:
        flat = baked(scene, scene.ranges, transforms, ids)
        out["flat_tris"] = flat.num_tris
        r = R.Renderer(flat, WIDTH, HEIGHT, SPP, MAXLEN, mapping="auto", gpu_bvh=2)
        tables = r.scene_table_pointers()
        out["given_ms"] = timed(lambda: r.update_geometry_device(tables["vertices"], tables["normals"], check=False), stream)
        out["given_status"] = r.update_status()[0]
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
    d, flat, f = r["deform"], r["flat"], r["refit"]
    ratio = lambda x, y: np.median(x) / np.median(y)
    row = lambda what, x, y: f"{what:44s} {spread(x):>30s} {spread(y):>30s} {ratio(x, y):10.4f}"
    lines = [f"# scripts/bench_instanced_deform.py --object {a.object} --instances {a.instances}; HIP events, ms, median [min, max] of "
             f"{REPS} after {WARMUP} warm-ups.",
             f"scene: {d['object_tris']} triangles x {a.instances} placements + ground + light = {flat['flat_tris']} triangles flat, "
             f"{d['instances']} instances; D = the plant ({d['refit_words'][0]} nodes, {d['refit_words'][1]} Tri1 records)",
             f"{'':44s} {'instanced, deform_objects':>30s} {'flat, update_geometry_device':>30s} {'ratio':>10s}",
             row("moved plant, given normals, ms", d["given_ms"], flat["given_ms"]),
             f"{'moved plant, smooth normals, ms':44s} {spread(d['smooth_ms']):>30s}",
             f"{'deform + new matrices in one call, ms':44s} {spread(d['with_matrices_ms']):>30s}",
             f"{'set_transforms alone, ms':44s} {spread(d['move_ms']):>30s}",
             f"status words: instanced {d['given_status']} / {d['smooth_status']}, flat {flat['given_status']}",
             f"{'':44s} {'refit_objects (one list)':>30s} {'loop of refit_bvh2_tri1':>30s} {'ratio':>10s}",
             row(f"{K_SMALL} objects of 12 triangles ({f['small_nodes']} nodes), ms", f["small_forest_ms"], f["small_loop_ms"]),
             row(f"the one plant ({f['plant_nodes']} nodes), ms", f["plant_forest_ms"], f["plant_loop_ms"]),
             "both refits leave the same bytes in the packed arrays (checked in the run)"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.output:
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        mode = "a" if Path(a.output).exists() else "w"
        with open(a.output, mode) as f_:
            f_.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
