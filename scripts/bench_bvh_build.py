"""Device BVH builder (rodent_amd.gpubuild, csrc/bvh_build.hip) against the host SBVH: build time, trace rate, tree quality.

For the atrium and the three 4.2 M-triangle stand-ins (scenes.scene_obj -> converter -> .rscene):
  * GPU build: device-event time of rodent_hip_build_bvh2_tri1 (median of --builds builds after 3 warm-ups), Mtriangles/s;
  * host SBVH: wall time of `converter` on the OBJ (it parses the OBJ too: an upper bound of the builder's own time);
  * traversal: Mrays/s of 1 Mi camera rays and 1 Mi random segments through hip_traverse_bvh2_tri1_async, default variant, closest
    hit, on both trees (median of 10 launches after 2 warm-ups);
  * quality: oracle steps (inner nodes + triangles) per ray on every 16th ray of both sets, and the SAH cost (tests/lbvh_model.py).
  * with --treelet-passes N > 0, the same for the optimised build (rodent_hip_build_bvh2_tri1_opt: N treelet passes + SAH leaf
    collapse, default costs) in the "opt" columns.

  * with --split-budget F [F ...] (and --treelet-passes N), the same for pre-split builds (rodent_hip_build_bvh2_tri1_split: budget F,
    --max-pieces K, N passes) in the "split F" columns: build ms, split ms (split build - unsplit build with the same passes),
    references, triangles split, leaves holding one triangle twice ("dup").

  * with --refit, beside each build time the device-event time of rodent_hip_refit_bvh2_tri1 on that tree (median of 20 after 3
    warm-ups; "refit ms"), and after the deformation of the refit tests (tests/refit_model.py deform, seed 1) the SAH cost of the
    refitted tree against a tree rebuilt from the moved vertices with the same options ("SAH refit" / "rebuilt").

  * with --refit-wide, nothing of the above: the host builder's BVH4 and BVH8 + Tri4 trees of every scene (bvh_extractor), the
    device-event time of rodent_hip_refit_bvh4_tri4 / _bvh8_tri4 on them (median of 20 after 3 warm-ups), beside it
    rodent_hip_refit_bvh2_tri1 on the BVH2 block of the same file and the wall time of bvh_extractor, which parses the OBJ and builds
    the three layouts side by side on three threads: an upper bound of one layout's host build.

  * with --collapse, nothing of the above: for the LBVH (max_leaf 4) and the 3-pass build (max_leaf 4) of every scene, the device-event
    time of rodent_hip_collapse_bvh2_tri1 into BVH4 and BVH8 (median of 20 after 3 warm-ups) beside the build before it, the wide
    nodes, packets, lane fill (records / (4 x packets)) and stack bound B, and Mrays/s (camera and random rays, closest and any hit,
    default variants) of the collapsed tree, of the host builder's tree of the same width (bvh_extractor) and of the BVH2 it came from.
    With --stack-limit L one more row per tree and width: the collapse under that limit (rodent_hip_collapse_bvh2_tri1_bounded) beside
    the one without: time with min and max, wide nodes, B, the BVH2's own H(0), closest-hit rates of both trees.

  * with --ploc R [R ...], nothing of the above: for every scene the LBVH, the 3-pass build and, per radius R, the PLOC build
    (rodent_hip_build_bvh2_tri1_ploc) with 0 and 1 treelet pass, all max_leaf 2 and timed in the same run: build ms (median [min, max]),
    nodes, depth, SAH cost (node / triangle cost 1.2 / 1.0), the clustering's iterations, the device-wide iterations launched and how
    many of them found one cluster left, kernel launches per build, Mrays/s of 1 Mi camera rays and 1 Mi random segments (closest hit,
    default variant) beside the host SBVH's; then the build time of the first radius over other numbers of device-wide iterations.

    python scripts/bench_bvh_build.py [--scenes atrium gallery crown plant] [--builds 20] [-o profiles/gpu_bvh_build.txt]
    python scripts/bench_bvh_build.py --treelet-passes 3 -o profiles/gpu_bvh_build_opt.txt
    python scripts/bench_bvh_build.py --treelet-passes 3 --split-budget 0.25 1 -o profiles/gpu_bvh_build_split.txt
    python scripts/bench_bvh_build.py --scenes atrium --treelet-passes 3 --split-budget 1 --refit -o profiles/gpu_bvh_refit.txt
    python scripts/bench_bvh_build.py --scenes atrium gallery --refit-wide -o profiles/gpu_bvh_refit_wide.txt
    python scripts/bench_bvh_build.py --scenes atrium gallery --collapse -o profiles/gpu_bvh_collapse.txt
    python scripts/bench_bvh_build.py --scenes atrium gallery --collapse --stack-limit 63 -o profiles/gpu_bvh_collapse_bounded.txt
    python scripts/bench_bvh_build.py --scenes atrium gallery --ploc 8 16 -o profiles/gpu_bvh_ploc.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from rodent_amd import abi, build, formats as F, gpubuild, raygen, scene as S, scenes  # noqa: E402


def event_ms(fn, warmup, reps, spread=False):
    """The median device-event time of fn() in ms; with `spread`: (median, min, max)."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return (float(np.median(times)), min(times), max(times)) if spread else float(np.median(times))


def tree_depth(nodes):
    """Node2 levels of a BVH2, level by level; every inner child index must be in range and referenced once."""
    child = nodes["child"].astype(np.int64)
    inner = child[child > 0] - 1
    assert (inner < len(nodes)).all() and len(np.unique(inner)) == len(inner) == len(nodes) - 1
    depth, frontier = 0, np.array([0])
    while len(frontier) and depth <= 64:
        depth += 1
        c = child[frontier].reshape(-1)
        frontier = c[c > 0] - 1
    return depth


def input_height(nodes, tris):
    """H(0) of a BVH2 (include/rodent_build.h, "Stack limit"): the bound of the tree left binary, by the model's level-wise pass."""
    import collapse_bounded_model as BM
    import collapse_model as M
    child = nodes["child"].astype(np.int64)
    flags, levels, run = M.guards(child, tris["prim_id"] < 0)
    assert flags == 0
    small, _ = M.small_subtrees(child, levels, run)
    return int(BM.heights(child, levels, small)[0])


def refit_wide_table(a):
    """--refit-wide: the refit of host-built BVH4 / BVH8 + Tri4 trees against the BVH2 refit and the host build."""
    build.build_all()
    lines = [f"# scripts/bench_bvh_build.py --refit-wide on {torch.cuda.get_device_name(0)}; refits: median of 20 after 3 warm-ups, device "
             "events around the enqueued operations, the tree's own vertices; host s: wall time of bvh_extractor (OBJ parse + BVH2, BVH4 "
             "and BVH8 side by side on three threads)",
             f"{'scene':>8} {'tris':>9} {'layout':>6} {'nodes':>8} {'leaf recs':>9} {'lanes':>9} | {'refit ms':>8} {'bvh2 ms':>8} "
             f"{'host s':>7} {'host / refit':>12}"]
    print("\n".join(lines), flush=True)
    scenes.DATA.mkdir(parents=True, exist_ok=True)
    stream = torch.cuda.current_stream()
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    for name in a.scenes:
        obj = scenes.scene_obj(name)
        stem = name.replace("/", "-")
        sc = S.convert(obj, scenes.DATA / f"{stem}.rscene")
        path = scenes.DATA / f"{stem}-refit-wide.bvh"
        t0 = time.perf_counter()
        subprocess.run([str(build.BIN_DIR / "bvh_extractor"), "-obj", str(obj), "-o", str(path)], check=True, stdout=subprocess.DEVNULL)
        host_s = time.perf_counter() - t0
        v, ix = torch.from_numpy(sc.vertices).cuda(), torch.from_numpy(sc.indices).cuda()
        ms = {}
        for width in (2, 4, 8):
            tree = abi.DeviceBvh.load(path, width)
            entry = getattr(abi.lib(), "rodent_hip_refit_bvh2_tri1" if width == 2 else f"rodent_hip_refit_bvh{width}_tri4")
            need = (abi.lib().rodent_hip_refit_scratch_bytes(tree.num_nodes, tree.num_tris) if width == 2 else
                    abi.lib().rodent_hip_refit_wide_scratch_bytes(width, tree.num_nodes, tree.num_tris))
            scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

            def one_refit():
                rc = entry(0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), sc.num_tris, tree.nodes.data_ptr(), tree.num_nodes,
                           tree.tris.data_ptr(), tree.num_tris, scratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
                assert rc == 0
            ms[width] = event_ms(one_refit, 3, 20)
            words = info.cpu().numpy().tolist()
            assert words[0] == tree.num_nodes and words[2:] == [0, 0], words
            if width > 2:
                row = (f"{name:>8} {sc.num_tris:>9} {'bvh' + str(width):>6} {tree.num_nodes:>8} {tree.num_tris:>9} {words[1]:>9} | "
                       f"{ms[width]:>8.3f} {ms[2]:>8.3f} {host_s:>7.1f} {host_s * 1e3 / ms[width]:>12.0f}")
                lines.append(row)
                print(row, flush=True)
            del tree, scratch
        del v, ix
        torch.cuda.empty_cache()
    Path(a.output).parent.mkdir(parents=True, exist_ok=True)
    Path(a.output).write_text("\n".join(lines) + "\n")


def collapse_table(a):
    """--collapse: the device collapse of device-built BVH2 trees into BVH4 / BVH8 + Tri4 against the build before it, and the collapsed
    trees' trace rates against the host builder's wide trees and the BVH2 they came from."""
    from oracle import binding as O
    build.build_all()
    lines = [f"# scripts/bench_bvh_build.py --collapse on {torch.cuda.get_device_name(0)}; builds and collapses: median of {a.builds} "
             "/ of 20 after 3 warm-ups, device events around the enqueued operations; fill: Tri1 records / (4 x packets); B: the stack "
             "bound info[3]; Mrays/s: 1 Mi camera rays / 1 Mi random segments, default variant, median of 10 launches after 2 warm-ups, "
             "closest / any hit: collapsed tree, host builder's tree of the same width, the BVH2 it came from",
             f"{'scene':>8} {'tris':>9} {'bvh2':>6} {'build ms':>8} {'nodes2':>8} | {'wide':>4} {'clps ms':>7} {'nodes':>8} {'packets':>8} "
             f"{'fill':>5} {'B':>3} {'host nodes':>10} {'host pk':>8} | {'cam closest':>17} {'cam any':>17} {'rand closest':>17} "
             f"{'rand any':>17}"]
    if a.stack_limit:
        lines.insert(1, f"# with --stack-limit {a.stack_limit}, a second row per tree and width: rodent_hip_collapse_bvh2_tri1_bounded under that "
                     "limit beside the collapse without one: ms = median [min, max] of the 20; H0: the BVH2's own bound H(0); same: the "
                     "two trees are equal byte for byte; Mrays/s closest hit: bounded tree / tree without a limit")
    print("\n".join(lines), flush=True)
    scenes.DATA.mkdir(parents=True, exist_ok=True)
    stream = torch.cuda.current_stream()
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    for name in a.scenes:
        obj = scenes.scene_obj(name)
        stem = name.replace("/", "-")
        sc = S.convert(obj, scenes.DATA / f"{stem}.rscene")
        path = scenes.DATA / f"{stem}-collapse.bvh"
        subprocess.run([str(build.BIN_DIR / "bvh_extractor"), "-obj", str(obj), "-o", str(path)], check=True, stdout=subprocess.DEVNULL)
        n = sc.num_tris
        v, ix = torch.from_numpy(sc.vertices).cuda(), torch.from_numpy(sc.indices).cuda()
        eye, d, up, fov = scenes.CAMERAS[name.split("/")[0]]
        lo, hi = sc.vertices[:, :3].min(0), sc.vertices[:, :3].max(0)
        ray_sets = {"cam": raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX),
                    "rand": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX)}
        rays_dev = {k: abi.to_device(r) for k, r in ray_sets.items()}
        hits = torch.empty((1 << 20) * 16, dtype=torch.uint8, device="cuda")

        def rates(tree):
            out = {}
            for rk, rd in rays_dev.items():
                for any_hit in (False, True):
                    ms = event_ms(lambda: abi.traverse_async(tree, rd, hits, 1 << 20, any_hit), 2, 10)
                    abi.check_errors()
                    out[rk, any_hit] = (1 << 20) / ms / 1e3
            return out
        for label, passes in (("lbvh", 0), ("3 pass", 3)):
            bvh = gpubuild.build_bvh2(v, ix, 4, treelet_passes=passes)
            copt = gpubuild.options(4, passes)

            def one_build():
                rc = abi.lib().rodent_hip_build_bvh2_tri1_opt(0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), n, C.byref(copt),
                                                              bvh.nodes.data_ptr(), bvh.tris.data_ptr(), bvh.scratch.data_ptr(),
                                                              info.data_ptr(), C.c_void_p(stream.cuda_stream))
                assert rc == 0
            build_ms = event_ms(one_build, 3, a.builds)
            assert info.cpu().numpy().tolist() == bvh.info.tolist()
            assert tree_depth(gpubuild.download(bvh)[0]) == bvh.depth <= 56          # checked before anything traces it
            rate2 = rates(bvh)
            for width in (4, 8):
                wide = gpubuild.collapse_wide(bvh, width)

                def one_collapse():
                    rc = abi.lib().rodent_hip_collapse_bvh2_tri1(0, width, bvh.nodes.data_ptr(), bvh.num_nodes, bvh.tris.data_ptr(),
                                                                 bvh.num_tris, wide.nodes.data_ptr(), wide.tris.data_ptr(),
                                                                 wide.scratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
                    assert rc == 0
                collapse_ms, collapse_min, collapse_max = event_ms(one_collapse, 3, 20, spread=True)
                assert info.cpu().numpy().tolist() == wide.info.tolist()
                B = int(wide.info[3])
                if B > 63:
                    # no guarantee from B: the CPU oracle looks at every 16th ray first, and nothing is traced past 64 entries
                    wn, wt = gpubuild.download_wide(wide)
                    peak = max(O.traverse(width, wn, wt, r[::16], any_hit=h, algo="gpu")[1]["max_stack"]
                               for r in ray_sets.values() for h in (False, True))
                    assert peak <= 64, f"{name} {label} bvh{width}: a stack of {peak} entries"
                host = abi.DeviceBvh.load(path, width)
                rate, rate_host = rates(wide), rates(host)
                cells = " ".join(f"{rate[k]:>5.0f} {rate_host[k]:>5.0f} {rate2[k]:>5.0f}" for k in
                                 (("cam", False), ("cam", True), ("rand", False), ("rand", True)))
                row = (f"{name:>8} {n:>9} {label:>6} {build_ms:>8.3f} {bvh.num_nodes:>8} | {'bvh' + str(width):>4} {collapse_ms:>7.3f} "
                       f"{wide.num_nodes:>8} {wide.num_tris:>8} {bvh.num_tris / (4 * wide.num_tris):>5.2f} {B:>3} {host.num_nodes:>10} "
                       f"{host.num_tris:>8} | {cells}")
                lines.append(row)
                print(row, flush=True)
                if a.stack_limit:
                    tight = gpubuild.collapse_wide(bvh, width, stack_limit=a.stack_limit)

                    def one_bounded():
                        rc = abi.lib().rodent_hip_collapse_bvh2_tri1_bounded(
                            0, width, a.stack_limit, bvh.nodes.data_ptr(), bvh.num_nodes, bvh.tris.data_ptr(), bvh.num_tris,
                            tight.nodes.data_ptr(), tight.tris.data_ptr(), tight.scratch.data_ptr(), info.data_ptr(),
                            C.c_void_p(stream.cuda_stream))
                        assert rc == 0
                    ms, lo_ms, hi_ms = event_ms(one_bounded, 3, 20, spread=True)
                    assert info.cpu().numpy().tolist() == tight.info.tolist()
                    h0 = input_height(*gpubuild.download(bvh))
                    assert tight.info[3] <= max(a.stack_limit, h0)
                    same = all(x.tobytes() == y.tobytes() for x, y in zip(gpubuild.download_wide(tight), gpubuild.download_wide(wide)))
                    rate_t = rate if same else rates(tight)       # equal bytes: the same tree, traced above
                    row = (f"{name:>8} {n:>9} {label:>6} {'L = ' + str(a.stack_limit):>17} | {'bvh' + str(width):>4} "
                           f"{ms:>7.3f} [{lo_ms:.3f}, {hi_ms:.3f}] no limit {collapse_ms:.3f} [{collapse_min:.3f}, {collapse_max:.3f}] "
                           f"nodes {tight.num_nodes} / {wide.num_nodes} fill {bvh.num_tris / (4 * tight.num_tris):.2f} "
                           f"B {int(tight.info[3])} / {B} H0 {h0} same {same} | "
                           f"cam {rate_t['cam', False]:.0f} / {rate['cam', False]:.0f} rand {rate_t['rand', False]:.0f} / {rate['rand', False]:.0f}")
                    lines.append(row)
                    print(row, flush=True)
                    del tight
                del wide, host
            del bvh
        del v, ix, rays_dev, hits
        torch.cuda.empty_cache()
    Path(a.output).parent.mkdir(parents=True, exist_ok=True)
    Path(a.output).write_text("\n".join(lines) + "\n")


def ploc_table(a):
    """--ploc: the PLOC topology stage against the LBVH and the 3-pass build of the same run: build time, tree quality, trace rate."""
    import lbvh_model as L
    build.build_all()
    lines = [f"# scripts/bench_bvh_build.py --ploc {' '.join(map(str, a.ploc))} on {torch.cuda.get_device_name(0)}; max_leaf 2; builds: "
             f"median [min, max] of {a.builds} after 3 warm-ups, device events around the enqueued operations; SAH: tests/lbvh_model.py "
             "sah_cost, node / triangle cost 1.2 / 1.0; iter: info[7]; wide: device-wide iterations launched (4 launches each), idle: those "
             "that found one cluster left; launches: kernels per build; Mrays/s: 1 Mi camera rays / 1 Mi random segments, closest hit, "
             "default variant, median of 10 launches after 2 warm-ups; x lbvh / x 3 pass / x sbvh: ratios to those rows",
             f"{'scene':>8} {'tris':>9} {'tree':>14} | {'build ms':>8} {'[min, max]':>18} {'x lbvh':>6} {'x 3 pass':>8} | {'nodes':>8} "
             f"{'depth':>5} {'SAH':>7} | {'iter':>4} {'wide':>4} {'idle':>4} {'launches':>8} | {'cam Mr/s':>8} {'x sbvh':>6} {'rand Mr/s':>9} "
             f"{'x sbvh':>6}"]
    print("\n".join(lines), flush=True)
    scenes.DATA.mkdir(parents=True, exist_ok=True)
    stream = torch.cuda.current_stream()
    info = torch.empty(8, dtype=torch.int32, device="cuda")
    l = abi.lib()
    for name in a.scenes:
        obj = scenes.scene_obj(name)
        sc = S.convert(obj, scenes.DATA / f"{name.replace('/', '-')}.rscene")
        n = sc.num_tris
        v, ix = torch.from_numpy(sc.vertices).cuda(), torch.from_numpy(sc.indices).cuda()
        eye, d, up, fov = scenes.CAMERAS[name.split("/")[0]]
        lo, hi = sc.vertices[:, :3].min(0), sc.vertices[:, :3].max(0)
        rays_dev = {"cam": abi.to_device(raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX)),
                    "rand": abi.to_device(raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX))}
        hits = torch.empty((1 << 20) * 16, dtype=torch.uint8, device="cuda")

        def rates(tree):
            out = {}
            for rk, rd in rays_dev.items():
                ms = event_ms(lambda: abi.traverse_async(tree, rd, hits, 1 << 20), 2, 10)
                abi.check_errors()
                out[rk] = (1 << 20) / ms / 1e3
            return out

        def timed(radius, passes, wide=-1):
            """(the tree, (median, min, max) ms) of one kind of build: radius 0 is the LBVH entry (0 passes) or the optimising one."""
            bvh = gpubuild.build_bvh2(v, ix, 2, treelet_passes=passes, ploc_radius=radius, wide_iterations=wide)
            copt = gpubuild.options(2, passes)
            cpl = abi.PlocOptions(radius, 0, wide)
            mesh = (0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), n)
            out = (bvh.nodes.data_ptr(), bvh.tris.data_ptr(), bvh.scratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))

            def one_build():
                if radius:
                    rc = l.rodent_hip_build_bvh2_tri1_ploc(*mesh, C.byref(copt), None, C.byref(cpl), *out)
                elif passes:
                    rc = l.rodent_hip_build_bvh2_tri1_opt(*mesh, C.byref(copt), *out)
                else:
                    rc = l.rodent_hip_build_bvh2_tri1(*mesh, 2, *out)
                assert rc == 0
            ms = event_ms(one_build, 3, a.builds, spread=True)
            assert info.cpu().numpy().tolist()[:len(bvh.info)] == bvh.info.tolist()
            return bvh, ms
        sbvh_rate = rates(abi.DeviceBvh(2, sc.nodes, sc.tris, 0))
        base = {}
        kinds = [("lbvh", 0, 0), ("3 pass", 0, 3)] + [(f"ploc {r} + {p}", r, p) for r in a.ploc for p in (0, 1)]
        for label, radius, passes in kinds:
            bvh, (ms, ms_lo, ms_hi) = timed(radius, passes)
            nodes, tris = gpubuild.download(bvh)
            assert tree_depth(nodes) == bvh.depth <= 56                 # checked before anything traces it
            rate = rates(bvh)
            if not radius:
                base[label] = ms
            # kernels: front 2, sort 13, leaves 1, then Karras 1 + LBVH tail 4 / optimising tail 5 + 2 per pass / PLOC 3 + 4 per
            # device-wide iteration + the optimising tail without k_explicit
            clog = int(n - 1).bit_length()
            wide = min(255, 4 * max(0, clog - 10)) if radius else 0
            launches = 16 + ((3 + 4 * wide + 4 + 2 * passes) if radius else (1 + 5 + 2 * passes) if passes else 5)
            it = int(bvh.info[7]) if radius else 0
            x = lambda k: f"{ms / base[k]:.2f}" if k in base else ""
            row = (f"{name:>8} {n:>9} {label:>14} | {ms:>8.3f} {'[%.3f, %.3f]' % (ms_lo, ms_hi):>18} {x('lbvh'):>6} {x('3 pass'):>8} | "
                   f"{bvh.num_nodes:>8} {bvh.depth:>5} {L.sah_cost(nodes, tris, 1.2, 1.0):>7.2f} | {it:>4} {wide:>4} {max(0, wide - it):>4} "
                   f"{launches:>8} | {rate['cam']:>8.0f} {rate['cam'] / sbvh_rate['cam']:>6.2f} {rate['rand']:>9.0f} "
                   f"{rate['rand'] / sbvh_rate['rand']:>6.2f}")
            lines.append(row)
            print(row, flush=True)
            del bvh
        row = (f"{name:>8} {n:>9} {'host sbvh':>14} | {'':>8} {'':>18} {'':>6} {'':>8} | {len(sc.nodes):>8} {tree_depth(sc.nodes):>5} "
               f"{L.sah_cost(sc.nodes, sc.tris, 1.2, 1.0):>7.2f} | {'':>4} {'':>4} {'':>4} {'':>8} | {sbvh_rate['cam']:>8.0f} {1.0:>6.2f} "
               f"{sbvh_rate['rand']:>9.0f} {1.0:>6.2f}")
        lines.append(row)
        print(row, flush=True)
        wide = min(255, 4 * max(0, int(n - 1).bit_length() - 10))
        sweep = []
        for w in sorted({wide // 2, 3 * wide // 4, wide, min(255, 3 * wide // 2)}):
            bvh, (ms, ms_lo, ms_hi) = timed(a.ploc[0], 0, w)
            sweep.append(f"{w}: {ms:.3f} [{ms_lo:.3f}, {ms_hi:.3f}]")
            del bvh
        row = f"# {name}: ploc {a.ploc[0]} + 0 build ms by device-wide iterations launched (the default is {wide}): " + "; ".join(sweep)
        lines.append(row)
        print(row, flush=True)
        del v, ix, rays_dev, hits
        torch.cuda.empty_cache()
    Path(a.output).parent.mkdir(parents=True, exist_ok=True)
    Path(a.output).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["atrium", "gallery", "crown", "plant"])
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--treelet-passes", type=int, default=0, help="also measure the optimised build with N passes (1 ... 3)")
    ap.add_argument("--split-budget", type=float, nargs="*", default=[], help="also measure pre-split builds with these budgets")
    ap.add_argument("--max-pieces", type=int, default=64)
    ap.add_argument("--refit", action="store_true", help="also time a refit of every built tree and compare refitted with rebuilt SAH")
    ap.add_argument("--refit-wide", action="store_true",
                    help="only time the refit of the host builder's BVH4 / BVH8 + Tri4 trees (beside: the BVH2 refit, the host build)")
    ap.add_argument("--collapse", action="store_true",
                    help="only time the collapse of device-built BVH2 trees into BVH4 / BVH8 + Tri4 and trace the collapsed trees")
    ap.add_argument("--stack-limit", type=int, default=0,
                    help="with --collapse: one more row per tree and width, the collapse under this stack limit (1 ... 63)")
    ap.add_argument("--ploc", type=int, nargs="+", default=[],
                    help="only compare the PLOC topology stage at these radii (0 and 1 treelet pass) with the LBVH and the 3-pass build")
    ap.add_argument("-o", "--output", default=str(ROOT / "profiles" / "gpu_bvh_build.txt"))
    a = ap.parse_args()
    if a.refit_wide:
        return refit_wide_table(a)
    if a.collapse:
        return collapse_table(a)
    if a.ploc:
        return ploc_table(a)
    from oracle import binding as O
    import lbvh_model as L
    import refit_model as RM
    build.build_all()
    lines = [f"# scripts/bench_bvh_build.py on {torch.cuda.get_device_name(0)}; builds: median of {a.builds} after 3 warm-ups, "
             "device events; traversal: default BVH2 variant, closest hit, median of 10 launches; steps: oracle, every 16th ray"]
    hdr = (f"{'scene':>8} {'tris':>9} | {'gpu ms':>7} {'Mtri/s':>7} {'nodes':>8} {'depth':>5} | {'sbvh s':>6} {'nodes':>8} | "
           f"{'prim Mr/s gpu':>13} {'sbvh':>6} | {'rand Mr/s gpu':>13} {'sbvh':>6} | {'steps prim gpu':>14} {'sbvh':>6} | "
           f"{'steps rand gpu':>14} {'sbvh':>6} | {'SAH gpu':>7} {'sbvh':>6}")
    P = a.treelet_passes
    if P:
        lines[0] += f"; opt: {P} treelet passes + SAH leaf collapse, max_leaf 2"
        hdr += (f" || {'opt ms':>7} {'nodes':>8} {'depth':>5} {'rej':>4} | {'prim Mr/s':>9} {'rand Mr/s':>9} | {'steps prim':>10} "
                f"{'rand':>6} | {'SAH':>6}")
    for B in a.split_budget:
        hdr += (f" || {'split ' + str(B):>10} {'split ms':>8} {'refs':>8} {'split':>7} {'dup':>6} {'depth':>5} | {'prim Mr/s':>9} "
                f"{'rand Mr/s':>9} | {'steps prim':>10} {'rand':>6} | {'SAH':>6}")
    if a.split_budget:
        lines[0] += f"; split: max_pieces {a.max_pieces}, {P} treelet passes, max_leaf 2"
    if a.refit:
        lines[0] += "; refit: median of 20 after 3 warm-ups, SAH after tests/refit_model.py deform(seed 1)"
        hdr += f" ||| {'refit of':>10} {'refit ms':>8} {'build ms':>8} {'SAH refit':>9} {'rebuilt':>7}"
    lines.append(hdr)
    print(hdr, flush=True)
    out_dir = scenes.DATA
    out_dir.mkdir(parents=True, exist_ok=True)
    for name in a.scenes:
        obj = scenes.scene_obj(name)
        rs = out_dir / f"{name.replace('/', '-')}.rscene"
        t0 = time.perf_counter()
        subprocess.run([str(build.BIN_DIR / "converter"), str(obj), "-o", str(rs)], check=True, stdout=subprocess.DEVNULL)
        host_s = time.perf_counter() - t0
        sc = S.Scene(rs)
        n = sc.num_tris
        v = torch.from_numpy(sc.vertices).cuda()
        ix = torch.from_numpy(sc.indices).cuda()
        bvh = gpubuild.build_bvh2(v, ix, 2)
        stream = torch.cuda.current_stream()
        info = torch.empty(4, dtype=torch.int32, device="cuda")

        def one_build():
            rc = abi.lib().rodent_hip_build_bvh2_tri1(0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), n, 2, bvh.nodes.data_ptr(),
                                                      bvh.tris.data_ptr(), bvh.scratch.data_ptr(), info.data_ptr(),
                                                      C.c_void_p(stream.cuda_stream))
            assert rc == 0
        build_ms = event_ms(one_build, 3, a.builds)
        assert info.cpu().numpy().tolist() == bvh.info.tolist()
        nodes, tris = gpubuild.download(bvh)
        sbvh = abi.DeviceBvh(2, sc.nodes, sc.tris, 0)
        kind = name.split("/")[0]
        eye, d, up, fov = scenes.CAMERAS[kind]
        lo, hi = sc.vertices[:, :3].min(0), sc.vertices[:, :3].max(0)
        ray_sets = {"primary": raygen.primary_rays(eye, d, up, fov, 1024, 1024, 0.0, scenes.PRIMARY_TMAX),
                    "random": raygen.random_rays(lo, hi, 1 << 20, 42, 0.0, scenes.RANDOM_TMAX)}
        trees = {"gpu": bvh, "sbvh": sbvh}
        host = {"gpu": (nodes, tris), "sbvh": (sc.nodes, sc.tris)}
        if P:
            opt = gpubuild.build_bvh2(v, ix, 2, treelet_passes=P)
            copt = gpubuild.options(2, P)

            def one_opt_build():
                rc = abi.lib().rodent_hip_build_bvh2_tri1_opt(0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), n, C.byref(copt),
                                                              opt.nodes.data_ptr(), opt.tris.data_ptr(), opt.scratch.data_ptr(),
                                                              info.data_ptr(), C.c_void_p(stream.cuda_stream))
                assert rc == 0
            opt_ms = event_ms(one_opt_build, 3, a.builds)
            assert info.cpu().numpy().tolist() == opt.info.tolist()
            host["opt"] = gpubuild.download(opt)
            assert tree_depth(host["opt"][0]) == opt.depth <= 56        # checked before anything traces it
            trees["opt"] = opt
        split_ms, split_info = {}, {}
        base_ms = opt_ms if P else build_ms
        for B in a.split_budget:
            sb = gpubuild.build_bvh2(v, ix, 2, treelet_passes=P, split_budget=B, max_pieces=a.max_pieces)
            copt, csp = gpubuild.options(2, P), gpubuild.split_options(B, a.max_pieces)
            sinfo = torch.empty(8, dtype=torch.int32, device="cuda")

            def one_split_build():
                rc = abi.lib().rodent_hip_build_bvh2_tri1_split(0, v.data_ptr(), len(sc.vertices), ix.data_ptr(), n, C.byref(copt),
                                                                C.byref(csp), sb.nodes.data_ptr(), sb.tris.data_ptr(),
                                                                sb.scratch.data_ptr(), sinfo.data_ptr(), C.c_void_p(stream.cuda_stream))
                assert rc == 0
            split_ms[B] = event_ms(one_split_build, 3, a.builds)
            assert sinfo.cpu().numpy().tolist() == sb.info.tolist()
            host[B] = gpubuild.download(sb)
            assert tree_depth(host[B][0]) == sb.depth <= 56          # checked before anything traces it
            ht = host[B][1]
            leaf = np.concatenate([[0], np.cumsum(ht["prim_id"][:-1] < 0)])
            pairs = np.unique(np.stack([leaf, ht["prim_id"] & 0x7FFFFFFF], 1), axis=0, return_counts=True)
            split_info[B] = (sb.num_tris, int(sb.info[5]), len(np.unique(pairs[0][pairs[1] > 1][:, 0])), sb.depth)
            trees[B] = sb
        rate, steps = {}, {}
        for rk, rays in ray_sets.items():
            rays_dev = abi.to_device(rays)
            hits = torch.empty(len(rays) * 16, dtype=torch.uint8, device="cuda")
            for tk, tree in trees.items():
                ms = event_ms(lambda: abi.traverse_async(tree, rays_dev, hits, len(rays)), 2, 10)
                abi.check_errors()
                rate[rk, tk] = len(rays) / ms / 1e3
            sub = rays[::16]
            for tk, (hn, ht) in host.items():
                steps[rk, tk] = O.ray_steps(hn, ht, sub).sum(1).mean()
        row = (f"{name:>8} {n:>9} | {build_ms:>7.3f} {n / build_ms / 1e3:>7.0f} {bvh.num_nodes:>8} {bvh.depth:>5} | {host_s:>6.1f} "
               f"{len(sc.nodes):>8} | {rate['primary', 'gpu']:>13.0f} {rate['primary', 'sbvh']:>6.0f} | {rate['random', 'gpu']:>13.0f} "
               f"{rate['random', 'sbvh']:>6.0f} | {steps['primary', 'gpu']:>14.1f} {steps['primary', 'sbvh']:>6.1f} | "
               f"{steps['random', 'gpu']:>14.1f} {steps['random', 'sbvh']:>6.1f} | {L.sah_cost(nodes, tris):>7.1f} "
               f"{L.sah_cost(sc.nodes, sc.tris):>6.1f}")
        if P:
            row += (f" || {opt_ms:>7.3f} {opt.num_nodes:>8} {opt.depth:>5} {int(opt.info[3]):>4} | {rate['primary', 'opt']:>9.0f} "
                    f"{rate['random', 'opt']:>9.0f} | {steps['primary', 'opt']:>10.1f} {steps['random', 'opt']:>6.1f} | "
                    f"{L.sah_cost(*host['opt']):>6.1f}")
        for B in a.split_budget:
            refs, nsplit, dup, depth = split_info[B]
            row += (f" || {split_ms[B]:>10.3f} {split_ms[B] - base_ms:>8.3f} {refs:>8} {nsplit:>7} {dup:>6} {depth:>5} | "
                    f"{rate['primary', B]:>9.0f} {rate['random', B]:>9.0f} | {steps['primary', B]:>10.1f} {steps['random', B]:>6.1f} | "
                    f"{L.sah_cost(*host[B]):>6.1f}")
        if a.refit:
            moved = torch.from_numpy(RM.deform(sc.vertices, sc.indices, seed=1)).cuda()
            kinds = [("gpu", bvh, build_ms, {})]
            if P:
                kinds.append(("opt", opt, opt_ms, {"treelet_passes": P}))
            kinds += [(f"split {B}", trees[B], split_ms[B], {"treelet_passes": P, "split_budget": B, "max_pieces": a.max_pieces})
                      for B in a.split_budget]
            for label, tree, ms, kw in kinds:
                rscratch = torch.empty(abi.lib().rodent_hip_refit_scratch_bytes(tree.num_nodes, tree.num_tris), dtype=torch.uint8,
                                       device="cuda")

                def one_refit(verts=v):
                    rc = abi.lib().rodent_hip_refit_bvh2_tri1(0, verts.data_ptr(), len(sc.vertices), ix.data_ptr(), n,
                                                              tree.nodes.data_ptr(), tree.num_nodes, tree.tris.data_ptr(), tree.num_tris,
                                                              rscratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
                    assert rc == 0
                refit_ms = event_ms(one_refit, 3, 20)            # with the build's own vertices: the same work, the tree keeps its shape
                assert info.cpu().numpy().tolist() == [tree.num_nodes, tree.num_tris, 0, 0]
                gpubuild.refit_bvh2(tree, moved, ix)
                rebuilt = gpubuild.build_bvh2(moved, ix, 2, **kw)
                row += (f" ||| {label:>10} {refit_ms:>8.3f} {ms:>8.3f} {L.sah_cost(*gpubuild.download(tree)):>9.1f} "
                        f"{L.sah_cost(*gpubuild.download(rebuilt)):>7.1f}")
                del rebuilt, rscratch
        trees.clear()
        lines.append(row)
        print(row, flush=True)
        del bvh, sbvh, v, ix
        torch.cuda.empty_cache()
    Path(a.output).parent.mkdir(parents=True, exist_ok=True)
    Path(a.output).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
