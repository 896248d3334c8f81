#!/usr/bin/env python
"""All objects of an instanced scene built in one launch list against the loop of per-object builds.

usage: python scripts/bench_build_objects.py [--object plant/1] [--parent-tree DIR] -o profiles/gpu_build_objects.txt

Measured, HIP events, ms, median [min, max] of 20 after 3 warm-ups, each case as instances.build_objects against
pack_objects([gpubuild.build_bvh2(...) for every object]); both forms must leave the same bytes (checked in the run):
  small    256 objects of 12 triangles (unit cubes side by side)
  plant    the one generated plant (--object)
  mid      64 distinct mid-sized objects (seeded soups of 2 000 to 9 875 triangles)
and, wall-clock ms around the call (it allocates and waits), Renderer(..., instances=...) creation of a 256-object scene (255 cubes and
one emissive quad) in this tree and, with --parent-tree (a built checkout of the parent commit), in that one.
Each step is a child process under its own time limit; the first failure ends the run.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TREE = Path(sys.argv[sys.argv.index("--tree") + 1]).resolve() if "--tree" in sys.argv else ROOT
sys.path.insert(0, str(TREE))
sys.path.insert(0, str(TREE / "scripts"))

from bench_instanced_deform import small_objects                                          # noqa: E402
from bench_instanced_render import HEIGHT, MAXLEN, SPP, WIDTH, material, part, quad          # noqa: E402
from bench_instances import REPS, WARMUP, object_mesh, spread, timed                         # noqa: E402

STEPS = (("small", 300), ("plant", 600), ("mid", 600), ("create", 300))
K_SMALL, K_MID = 256, 64


def mid_objects(k=K_MID):
    rng = np.random.default_rng(17)
    vertices, indices, rows, base = [], [], [], 0
    for o in range(k):
        n = 2000 + 125 * o
        centre = rng.uniform(-20, 20, (n, 1, 3))
        v = np.zeros((3 * n, 4), np.float32)
        v[:, :3] = (centre + rng.normal(0, 0.5, (n, 3, 3))).reshape(-1, 3)
        ix = np.zeros((n, 4), np.int32)
        ix[:, :3] = np.arange(3 * n).reshape(-1, 3) + base
        rows.append((sum(len(i) for i in indices), n))
        vertices.append(v); indices.append(ix)
        base += 3 * n
    return np.concatenate(vertices), np.concatenate(indices), np.int32(rows)


def list_against_loop(out, v, ix, rows, stream):
    import torch
    from rodent_amd import gpubuild, instances as I
    vd, ixd = torch.from_numpy(v).cuda(), torch.from_numpy(ix).cuda()
    made = {}

    def one_list():
        made["list"] = I.build_objects(vd, ixd, rows, max_leaf=2)

    def loop():
        made["loop"] = I.pack_objects([gpubuild.build_bvh2(vd, ixd[int(f): int(f + n)], max_leaf=2) for f, n in rows])
    out["list_ms"], out["loop_ms"] = timed(one_list, stream), timed(loop, stream)
    a, b = made["list"], made["loop"]
    assert a.table.tobytes() == b.table.tobytes(), "the tables differ"
    assert torch.equal(a.nodes, b.nodes) and torch.equal(a.tris, b.tris), "the one-list build leaves other bytes than the loop"
    out["objects"], out["tris"], out["nodes"] = len(rows), int(a.num_tris), int(a.num_nodes)


def cube_scene(k=K_SMALL):
    """(ObjectScene, transforms, ids): k - 1 unit cubes side by side and one emissive quad above them."""
    from rodent_amd import instances as I
    v, ix, _ = small_objects(1)
    objects = [part(v, ix, material((0.5, 0.5, 0.5))) for _ in range(k - 1)] + [part(*quad(False), material((0, 0, 0), True), True)]
    t = np.zeros((k, 3, 4), np.float32)
    t[:, 0, 0] = t[:, 1, 1] = t[:, 2, 2] = 1.0
    t[:, 0, 3] = 2.0 * np.arange(k)
    t[k - 1] = [[2.0 * k, 0, 0, k], [0, 1, 0, 5.0], [0, 0, 2.0 * k, 0]]
    return I.concat_scenes(objects), t.reshape(k, 12), np.arange(k, dtype=np.int32)


def step(name, a):
    import torch
    out = {}
    if name == "create":
        from rodent_amd import render as R
        scene, transforms, ids = cube_scene()
        times = []
        for _ in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = R.Renderer(scene, WIDTH, HEIGHT, SPP, MAXLEN, instances=(scene.ranges, transforms, ids))
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
            r.close()
        out["create_ms"], out["objects"] = times[WARMUP:], len(ids)
        return out
    stream = torch.cuda.current_stream()
    if name == "small":
        v, ix, rows = small_objects(K_SMALL)
    elif name == "plant":
        v, ix = object_mesh(a.object)
        rows = np.int32([[0, len(ix)]])
    else:
        v, ix, rows = mid_objects()
    list_against_loop(out, v, ix, rows, stream)
    return out


def run_step(name, limit, a, tree=None):
    cmd = [sys.executable, __file__, "--object", a.object, "--step", name] + (["--tree", str(tree)] if tree else [])
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"step {name} failed (no result within {limit} s): nothing further is run", file=sys.stderr)
        return None
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(p.stdout + p.stderr, file=sys.stderr)
        print(f"step {name} failed (exit status {p.returncode}): nothing further is run", file=sys.stderr)
        return None
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--object", default="plant/1", help="scenes.py's generated kind / detail (plant/1, crown/1)")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: scene creation is measured there too")
    ap.add_argument("--tree", help="(internal) import rodent_amd and the helper scripts from this tree")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one step and print its figures as JSON")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a)))
        return 0
    r = {}
    for name, limit in STEPS:
        r[name] = run_step(name, limit, a)
        if r[name] is None:
            return 1
    parent = None
    if a.parent_tree:
        parent = run_step("create", 300, a, a.parent_tree)
        if parent is None:
            return 1
    ratio = lambda x, y: np.median(x) / np.median(y)
    what = {"small": "{objects} objects of 12 triangles ({nodes} nodes)", "plant": "the one plant ({tris} triangles, {nodes} nodes)",
            "mid": "{objects} mid-sized objects ({tris} triangles, {nodes} nodes)"}
    lines = [f"# scripts/bench_build_objects.py --object {a.object}; HIP events, ms, median [min, max] of {REPS} after {WARMUP} warm-ups.",
             f"{'':58s} {'build_objects (one list)':>30s} {'loop of build_bvh2 + pack_objects':>34s} {'ratio':>10s}"]
    for name in ("small", "plant", "mid"):
        c = r[name]
        lines.append(f"{what[name].format(**c) + ', ms':58s} {spread(c['list_ms']):>30s} {spread(c['loop_ms']):>34s} "
                     f"{ratio(c['list_ms'], c['loop_ms']):10.4f}")
    lines.append("both forms leave the same table, Node2 and Tri1 bytes (checked in the run)")
    c = r["create"]
    lines.append(f"Renderer(..., instances=...) creation, {c['objects']} objects, wall-clock ms: this tree {spread(c['create_ms'])}"
                 + (f"; the parent commit's build {spread(parent['create_ms'])}; ratio {ratio(c['create_ms'], parent['create_ms']):.4f}"
                    if parent else "; the parent commit's build: not measured"))
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
