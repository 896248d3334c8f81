"""BVH2 / Tri1 hierarchies built on the GPU (the LBVH builder of csrc/bvh_build.hip, C ABI include/rodent_build.h).

    bvh = build_bvh2(vertices, indices)            # numpy arrays or CUDA tensors, (n, 3) or (n, 4)
    bvh = build_bvh2(vertices, indices, treelet_passes=2)   # + treelet restructuring and an SAH leaf collapse
    hits = abi.traverse(bvh, rays)

The result is a pure function of the inputs, byte for byte.  As a tool:

    python -m rodent_amd.gpubuild scene.rscene -o out.bvh [--max-leaf N] [--treelet-passes N]

writes a .bvh holding the BVH2_TRI1 block of the scene's mesh (bench_traversal reads it).
"""
from __future__ import annotations

import argparse
import ctypes as C

import numpy as np
import torch

from . import abi, formats as F

MAX_TRIS = 1 << 25
MAX_LEAF = 8
MAX_TREELET_PASSES = 3
NODE_COST, TRI_COST = 1.2, 1.0         # RODENT_BUILD_DEFAULT_NODE_COST / _TRI_COST
INFO_WORDS = 4
BAD_INDEX, NON_FINITE = 1, 2
_ERRORS = {-1: "num_tris outside [1, 2^25]", -2: "max_leaf outside [1, 8]", -3: "no vertices", -4: "NULL pointer",
           -5: "no such device", -6: "launch failed", -8: "treelet_passes outside [0, 3]", -9: "node_cost / tri_cost outside (0, 1e6]"}


class BuildError(RuntimeError):
    pass


def _columns4(a, dtype, dev):
    """(n, 3) or (n, 4) numpy array / tensor -> contiguous (n, 4) CUDA tensor of `dtype`; a missing 4th column is 0."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] not in (3, 4):
        raise ValueError(f"expected an (n, 3) or (n, 4) array, got shape {tuple(t.shape)}")
    t = t.to(device=f"cuda:{dev}", dtype=dtype)
    if t.shape[1] == 3:
        t = torch.cat([t, torch.zeros((t.shape[0], 1), dtype=dtype, device=t.device)], 1)
    return t.contiguous()


def options(max_leaf=2, treelet_passes=0, node_cost=NODE_COST, tri_cost=TRI_COST) -> abi.BuildOptions:
    """A checked RodentBuildOptions; raises BuildError on values the library would refuse."""
    if not 1 <= max_leaf <= MAX_LEAF:
        raise BuildError(f"max_leaf = {max_leaf}: outside [1, 8]")
    if not 0 <= treelet_passes <= MAX_TREELET_PASSES:
        raise BuildError(f"treelet_passes = {treelet_passes}: outside [0, 3]")
    opt = abi.BuildOptions(int(max_leaf), int(treelet_passes), float(node_cost), float(tri_cost))
    if not all(0.0 < c <= 1e6 for c in (opt.node_cost, opt.tri_cost)):
        raise BuildError(f"node_cost = {node_cost}, tri_cost = {tri_cost}: outside (0, 1e6]")
    return opt


def build_bvh2(vertices, indices, max_leaf=2, dev=0, stream=None, scratch=None, out=None, treelet_passes=0, node_cost=NODE_COST,
               tri_cost=TRI_COST) -> abi.DeviceBvh:
    """Builds the BVH2 / Tri1 hierarchy of the triangles `indices` (v0 v1 v2 [geometry id]; 3 columns: geometry id 0) over
    `vertices` (x y z [w]) on device `dev`, on `stream` (torch stream, None = the current one).  Returns an abi.DeviceBvh whose
    `depth` and `info` are set.  Raises BuildError on invalid arguments and on the device's error flags (an index outside the
    vertex array, a non-finite coordinate).

    scratch / out: reuse the scratch tensor / the node and triangle tensors of an earlier result (rebuild in place); they must be
    large enough.
    treelet_passes = 1 ... 3: restructure the LBVH's treelets and collapse its leaves by SAH cost (node_cost, tri_cost; max_leaf is
    then the largest leaf allowed, not a threshold); info[3] counts the topologies the depth rule rejected.  0: the LBVH as it is."""
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    v = _columns4(vertices, torch.float32, dev)
    ix = _columns4(indices, torch.int32, dev)
    n, nv = ix.shape[0], v.shape[0]
    if not 1 <= n <= MAX_TRIS:
        raise BuildError(f"num_tris = {n}: outside [1, 2^25]")
    opt = options(max_leaf, treelet_passes, node_cost, tri_cost)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    l = abi.lib()
    need = l.rodent_hip_build_opt_scratch_bytes(n, C.byref(opt))
    cuda = f"cuda:{dev}"
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    if out is None:
        nodes = torch.empty(max(1, n - 1) * F.NODE2.itemsize, dtype=torch.uint8, device=cuda)
        tris = torch.empty(n * F.TRI1.itemsize, dtype=torch.uint8, device=cuda)
    else:
        nodes, tris = out.nodes, out.tris
        if (nodes.numel() * nodes.element_size() < max(1, n - 1) * F.NODE2.itemsize
                or tris.numel() * tris.element_size() < n * F.TRI1.itemsize):
            raise ValueError("build_bvh2: the buffers of `out` are too small for this mesh")
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    # the caller's tensors may come from another stream: make this one wait for the inputs
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        entry = "rodent_hip_build_bvh2_tri1_opt" if treelet_passes else "rodent_hip_build_bvh2_tri1"
        if treelet_passes:
            rc = l.rodent_hip_build_bvh2_tri1_opt(dev, v.data_ptr(), nv, ix.data_ptr(), n, C.byref(opt), nodes.data_ptr(),
                                                  tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
        else:
            rc = l.rodent_hip_build_bvh2_tri1(dev, v.data_ptr(), nv, ix.data_ptr(), n, int(max_leaf), nodes.data_ptr(),
                                              tris.data_ptr(), scratch.data_ptr(), info.data_ptr(), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise BuildError(f"{entry}: {_ERRORS.get(rc, rc)}")
        for t in (v, ix, scratch, info):
            t.record_stream(stream)
        words = info.cpu().numpy()
    if words[2]:
        what = [s for bit, s in ((BAD_INDEX, "vertex index outside the vertex array"), (NON_FINITE, "non-finite vertex coordinate"))
                if words[2] & bit]
        raise BuildError(f"{entry}: " + ", ".join(what))
    bvh = abi.DeviceBvh.from_tensors(2, nodes, tris, int(words[0]), n, dev)
    bvh.depth, bvh.info, bvh.scratch = int(words[1]), words.copy(), scratch
    return bvh


def download(bvh: abi.DeviceBvh):
    """(nodes NODE2, tris TRI1) host copies of a BVH2 / Tri1 DeviceBvh."""
    nodes = bvh.nodes.view(torch.uint8)[: bvh.num_nodes * F.NODE2.itemsize].cpu().numpy().view(F.NODE2).copy()
    tris = bvh.tris.view(torch.uint8)[: bvh.num_tris * F.TRI1.itemsize].cpu().numpy().view(F.TRI1).copy()
    return nodes, tris


def main(argv=None):
    from .scene import Scene
    ap = argparse.ArgumentParser(prog="python -m rodent_amd.gpubuild", description="BVH2 / Tri1 of a .rscene's mesh, built on the GPU")
    ap.add_argument("scene", help=".rscene file (converter)")
    ap.add_argument("-o", "--output", required=True, help=".bvh file to write (BVH2_TRI1 block)")
    ap.add_argument("--max-leaf", type=int, default=2, help="largest leaf (1 ... 8, default 2)")
    ap.add_argument("--treelet-passes", type=int, default=0,
                    help="treelet restructuring passes + SAH leaf collapse (0 ... 3, default 0: the LBVH as it is)")
    ap.add_argument("--dev", type=int, default=0)
    a = ap.parse_args(argv)
    sc = Scene(a.scene)
    bvh = build_bvh2(sc.vertices, sc.indices, a.max_leaf, a.dev, treelet_passes=a.treelet_passes)
    nodes, tris = download(bvh)
    F.write_bvh(a.output, [(F.BVH2_TRI1, nodes, tris)])
    print(f"{a.output}: {len(tris)} triangles, {len(nodes)} nodes, depth {bvh.depth}")


if __name__ == "__main__":
    main()
