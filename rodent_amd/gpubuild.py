"""BVH2 / Tri1 hierarchies built on the GPU (the LBVH builder of csrc/bvh_build.hip, C ABI include/rodent_build.h), and their collapse
into BVH4 / BVH8 + Tri4.

    bvh = build_bvh2(vertices, indices)            # numpy arrays or CUDA tensors, (n, 3) or (n, 4)
    bvh = build_bvh2(vertices, indices, treelet_passes=2)   # + treelet restructuring and an SAH leaf collapse
    bvh = build_bvh2(vertices, indices, treelet_passes=3, split_budget=1.0)   # + triangle pre-splitting (bvh.num_tris references)
    hits = abi.traverse(bvh, rays)
    refit_bvh2(bvh, moved_vertices, indices)       # the vertices moved: new boxes and Tri1 records in place, the topology stays
    refit_wide(wide, moved_vertices, indices)      # the same for a BVH4 / BVH8 + Tri4 DeviceBvh (collapsed, or of the host builder)
    wide = collapse_wide(bvh, 8)                   # the BVH2 collapsed into BVH8 / Tri4 on the device; wide.info[3]: its stack bound
    wide = build_wide(vertices, indices, 8, max_leaf=4, treelet_passes=3)    # build_bvh2 then collapse_wide; wide.bvh2 is the BVH2
    wide = build_wide(vertices, indices, 8, stack_limit=63)    # a tree no ray can overflow the traversal stack of: info[3] <= 63
    bvh = build_bvh2(vertices, indices, ploc_radius=16, treelet_passes=1)    # topology by locally-ordered clustering (PLOC)

The result is a pure function of the inputs, byte for byte.  As a tool:

    python -m rodent_amd.gpubuild scene.rscene -o out.bvh [--max-leaf N] [--treelet-passes N] [--split-budget F [--max-pieces K]]
                                  [--ploc-radius R [--depth-limit D]] [--width 4] [--width 8] [--stack-limit L]

writes a .bvh holding the BVH2_TRI1 block of the scene's mesh and, for every --width, its collapsed BVH4_TRI4 / BVH8_TRI4 block
(bench_traversal reads them), collapsed under the stack limit L when one is given.
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
SPLIT_INFO_WORDS = 8                   # + [4] Tri1 count (references) [5] triangles split [6] splits allotted but not made [7] 0
MAX_PIECES, MAX_SPLIT_BUDGET = 64, 4.0
BAD_INDEX, NON_FINITE, BAD_TOPOLOGY = 1, 2, 4
ERR_SPLIT, ERR_NUM_NODES, ERR_WIDTH, ERR_STACK_LIMIT, ERR_PLOC = -10, -11, -12, -13, -16
MAX_STACK_LIMIT = 63
MAX_PLOC_RADIUS, MAX_DEPTH = 64, 56    # RODENT_BUILD_MAX_PLOC_RADIUS / _MAX_DEPTH
_ERRORS = {-1: "num_tris outside [1, 2^25]", -2: "max_leaf outside [1, 8]", -3: "no vertices", -4: "NULL pointer",
           -5: "no such device", -6: "launch failed", -8: "treelet_passes outside [0, 3]", -9: "node_cost / tri_cost outside (0, 1e6]",
           ERR_SPLIT: "split budget outside [0, 4] or max_pieces outside [1, 64]", ERR_NUM_NODES: "a hierarchy without nodes or triangles",
           ERR_WIDTH: "width other than 4 or 8", ERR_STACK_LIMIT: "stack_limit outside [0, 63]",
           -14: "num_instances outside [1, 2^22]", -15: "no objects",      # RODENT_TLAS_ERR_* (rodent_amd/instances.py)
           ERR_PLOC: "PLOC radius outside [1, 64], depth_limit outside [0, 56] or below ceil(log2 references) or below 56 with "
                     "treelet passes, or wide_iterations outside [-1, 255]"}
_FLAGS = ((BAD_INDEX, "vertex index outside the vertex array"), (NON_FINITE, "non-finite vertex coordinate"),
          (BAD_TOPOLOGY, "malformed hierarchy (child id or prim_id out of range, leaf without end bit, node with two parents)"))


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


def _mesh(vertices, indices, dev, stream):
    """What build_bvh2 and refit_bvh2 start with: the GPU check, the (n, 4) device tensors, the num_tris range, the stream default.
    Returns (v, ix, stream)."""
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    v, ix = _columns4(vertices, torch.float32, dev), _columns4(indices, torch.int32, dev)
    if not 1 <= ix.shape[0] <= MAX_TRIS:
        raise BuildError(f"num_tris = {ix.shape[0]}: outside [1, 2^25]")
    return v, ix, torch.cuda.current_stream(dev) if stream is None else stream


def _enqueue(entry, dev, stream, info, used, *args):
    """Calls `entry`(dev, *args, info, stream) on `stream` once it has waited for the caller's current stream (the tensors may come from
    there), records `used` and `info` on it and returns the info words on the host.  Raises BuildError when the entry refuses."""
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        rc = getattr(abi.lib(), entry)(dev, *args, info.data_ptr(), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise BuildError(f"{entry}: {_ERRORS.get(rc, rc)}")
        for t in (*used, info):
            t.record_stream(stream)
        return info.cpu().numpy()


def _raise_flags(entry, words):
    if words[2]:
        raise BuildError(f"{entry}: " + ", ".join(s for bit, s in _FLAGS if words[2] & bit))


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


def split_options(budget=0.0, max_pieces=MAX_PIECES) -> abi.SplitOptions:
    """A checked RodentSplitOptions; raises BuildError on values the library would refuse."""
    sp = abi.SplitOptions(float(budget), int(max_pieces))
    if not 0.0 <= sp.budget <= MAX_SPLIT_BUDGET:
        raise BuildError(f"split budget = {budget}: outside [0, 4]")
    if not 1 <= max_pieces <= MAX_PIECES:
        raise BuildError(f"max_pieces = {max_pieces}: outside [1, 64]")
    return sp


def ploc_options(radius, depth_limit=0, wide_iterations=-1) -> abi.PlocOptions:
    """A checked RodentPlocOptions; raises BuildError on values the library would refuse whatever the mesh."""
    if not 1 <= radius <= MAX_PLOC_RADIUS:
        raise BuildError(f"ploc_radius = {radius}: outside [1, 64]")
    if not 0 <= depth_limit <= MAX_DEPTH:
        raise BuildError(f"depth_limit = {depth_limit}: outside [0, 56]")
    if not -1 <= wide_iterations <= 255:
        raise BuildError(f"wide_iterations = {wide_iterations}: outside [-1, 255]")
    return abi.PlocOptions(int(radius), int(depth_limit), int(wide_iterations))


def build_bvh2(vertices, indices, max_leaf=2, dev=0, stream=None, scratch=None, out=None, treelet_passes=0, node_cost=NODE_COST,
               tri_cost=TRI_COST, split_budget=0.0, max_pieces=None, ploc_radius=0, depth_limit=0, wide_iterations=-1) -> abi.DeviceBvh:
    """Builds the BVH2 / Tri1 hierarchy of the triangles `indices` (v0 v1 v2 [geometry id]; 3 columns: geometry id 0) over
    `vertices` (x y z [w]) on device `dev`, on `stream` (torch stream, None = the current one).  Returns an abi.DeviceBvh whose
    `depth` and `info` are set.  Raises BuildError on invalid arguments and on the device's error flags (an index outside the
    vertex array, a non-finite coordinate).

    scratch / out: reuse the scratch tensor / the node and triangle tensors of an earlier result (rebuild in place); they must be
    large enough.
    treelet_passes = 1 ... 3: restructure the LBVH's treelets and collapse its leaves by SAH cost (node_cost, tri_cost; max_leaf is
    then the largest leaf allowed, not a threshold); info[3] counts the topologies the depth rule rejected.  0: the LBVH as it is.
    split_budget > 0 or max_pieces given: pre-split the triangles first (rodent_hip_build_bvh2_tri1_split; up to split_budget * n
    extra references, at most max_pieces (default 64) per triangle); bvh.num_tris is then the reference count info[4], and info has
    8 words.
    ploc_radius = 1 ... 64: the topology comes from locally-ordered clustering over that many Morton neighbours to either side
    (rodent_hip_build_bvh2_tri1_ploc) instead of the LBVH's; treelet_passes (0: clustering + SAH leaf collapse) and the split options
    act on it as above.  depth_limit: the most Node2 levels (0 = 56; below 56 only with treelet_passes = 0); wide_iterations: scheduling
    only (-1: the library's choice).  info has 8 words, info[7] counts the clustering's iterations.  0: the entries above."""
    v, ix, stream = _mesh(vertices, indices, dev, stream)
    n, nv = ix.shape[0], v.shape[0]
    opt = options(max_leaf, treelet_passes, node_cost, tri_cost)
    splitting = bool(split_budget) or max_pieces is not None
    sp = split_options(split_budget, MAX_PIECES if max_pieces is None else max_pieces) if splitting else None
    if not ploc_radius and (depth_limit or wide_iterations != -1):
        raise BuildError("depth_limit and wide_iterations need ploc_radius")
    l = abi.lib()
    # the entry and its option arguments, its scratch bytes, the Tri1 records it may write, its info words
    if ploc_radius:
        pl = ploc_options(ploc_radius, depth_limit, wide_iterations)
        entry, args, info_words = "rodent_hip_build_bvh2_tri1_ploc", (C.byref(opt), C.byref(sp) if splitting else None, C.byref(pl)), 8
        need = l.rodent_hip_build_ploc_scratch_bytes(n, *args)
        if need < 0:
            raise BuildError(f"{entry}: {_ERRORS[ERR_PLOC]}")
        refs = l.rodent_hip_build_split_max_refs(n, C.byref(sp)) if splitting else n
    elif splitting:
        entry, args, info_words = "rodent_hip_build_bvh2_tri1_split", (C.byref(opt), C.byref(sp)), SPLIT_INFO_WORDS
        need, refs = l.rodent_hip_build_split_scratch_bytes(n, *args), l.rodent_hip_build_split_max_refs(n, C.byref(sp))
    else:
        entry, args = (("rodent_hip_build_bvh2_tri1_opt", (C.byref(opt),)) if treelet_passes else
                       ("rodent_hip_build_bvh2_tri1", (int(max_leaf),)))
        info_words = INFO_WORDS
        need, refs = l.rodent_hip_build_opt_scratch_bytes(n, C.byref(opt)), n
    cuda = f"cuda:{dev}"
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    if out is None:
        nodes = torch.empty(max(1, refs - 1) * F.NODE2.itemsize, dtype=torch.uint8, device=cuda)
        tris = torch.empty(refs * F.TRI1.itemsize, dtype=torch.uint8, device=cuda)
    else:
        nodes, tris = out.nodes, out.tris
        if (nodes.numel() * nodes.element_size() < max(1, refs - 1) * F.NODE2.itemsize
                or tris.numel() * tris.element_size() < refs * F.TRI1.itemsize):
            raise ValueError("build_bvh2: the buffers of `out` are too small for this mesh")
    info = torch.empty(info_words, dtype=torch.int32, device=cuda)
    words = _enqueue(entry, dev, stream, info, (v, ix, scratch), v.data_ptr(), nv, ix.data_ptr(), n, *args, nodes.data_ptr(),
                     tris.data_ptr(), scratch.data_ptr())
    _raise_flags(entry, words)
    bvh = abi.DeviceBvh.from_tensors(2, nodes, tris, int(words[0]), int(words[4]) if splitting or ploc_radius else n, dev)
    bvh.depth, bvh.info, bvh.scratch = int(words[1]), words.copy(), scratch
    return bvh


def _refit(entry, need, bvh, vertices, indices, stream, scratch):
    """refit_bvh2 and refit_wide after their width checks: `entry` on `bvh` with at least `need` bytes of scratch."""
    dev = bvh.dev
    v, ix, stream = _mesh(vertices, indices, dev, stream)
    if need < 0:
        raise BuildError(f"{entry}: {_ERRORS[ERR_NUM_NODES]}")
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=f"cuda:{dev}")
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=f"cuda:{dev}")
    words = _enqueue(entry, dev, stream, info, (v, ix, scratch, bvh.nodes, bvh.tris), v.data_ptr(), v.shape[0], ix.data_ptr(), ix.shape[0],
                     bvh.nodes.data_ptr(), bvh.num_nodes, bvh.tris.data_ptr(), bvh.num_tris, scratch.data_ptr())
    bvh.info, bvh.scratch = words.copy(), scratch
    _raise_flags(entry, words)
    if words[0] != bvh.num_nodes:
        raise BuildError(f"{entry}: malformed hierarchy ({words[0]} of {bvh.num_nodes} nodes completed)")
    return bvh


def refit_bvh2(bvh: abi.DeviceBvh, vertices, indices, stream=None, scratch=None) -> abi.DeviceBvh:
    """Refits the BVH2 / Tri1 hierarchy `bvh` in place to moved `vertices` (rodent_hip_refit_bvh2_tri1): new boxes and Tri1 records,
    the same topology.  `indices` is the triangle table the hierarchy's prim ids refer to; arrays and stream as in build_bvh2.  `bvh` may
    come from build_bvh2 (any options) or from a host builder.  Returns `bvh` itself with `info` replaced ([0] nodes completed, [1]
    records rewritten, [2] flags).  Raises BuildError on invalid arguments, on the device's flags (an index outside the vertex array, a
    non-finite coordinate, a malformed hierarchy) and when not every node was completed.

    Refitted with the vertices it was built from, an unsplit build_bvh2 tree keeps its bytes.  A split tree's references get their
    whole triangles' boxes: correct, but looser than the clipped boxes the builder stored."""
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    if bvh.width != 2:
        raise ValueError("refit_bvh2: a BVH2 / Tri1 hierarchy is needed")
    need = abi.lib().rodent_hip_refit_scratch_bytes(bvh.num_nodes, bvh.num_tris)
    return _refit("rodent_hip_refit_bvh2_tri1", need, bvh, vertices, indices, stream, scratch)


def refit_wide(bvh: abi.DeviceBvh, vertices, indices, stream=None, scratch=None) -> abi.DeviceBvh:
    """refit_bvh2 for a BVH4 / BVH8 + Tri4 hierarchy (rodent_hip_refit_bvh4_tri4 / _bvh8_tri4; bvh.num_tris counts its Tri4 packets):
    new slot boxes and new v0 / e1 / e2 / n columns in the valid lanes of every packet, the same topology.  Arguments, result and
    errors as refit_bvh2; info[1] counts the lanes rewritten."""
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    if bvh.width not in (4, 8):
        raise ValueError("refit_wide: a BVH4 / BVH8 + Tri4 hierarchy is needed")
    need = abi.lib().rodent_hip_refit_wide_scratch_bytes(bvh.width, bvh.num_nodes, bvh.num_tris)
    return _refit(f"rodent_hip_refit_bvh{bvh.width}_tri4", need, bvh, vertices, indices, stream, scratch)


def collapse_wide(bvh2: abi.DeviceBvh, width, stream=None, scratch=None, stack_limit=0) -> abi.DeviceBvh:
    """Collapses the BVH2 / Tri1 hierarchy `bvh2` (of build_bvh2, any options, or of a host builder) into a new BVH4 / BVH8 + Tri4
    DeviceBvh of `width` slots to a node (rodent_hip_collapse_bvh2_tri1); `bvh2` is only read.  The result's num_tris counts its Tri4
    packets, as for a host builder's wide tree, and its `info` holds [0] wide nodes [1] packets [2] flags [3] the stack bound B: no ray's
    traversal stack holds more than B entries, so B <= 63 rules an overflow out (B is not checked here).  Stream and scratch as in
    build_bvh2.  Raises BuildError on a malformed hierarchy.

    stack_limit = L in 1 ... 63 (rodent_hip_collapse_bvh2_tri1_bounded): the growth stops widening where that would take B past L, so
    B <= max(L, H(0)), H(0) being the bound of the BVH2 itself: 63 gives B <= 63 for every build_bvh2 tree.  0: no limit."""
    if not torch.cuda.is_available():
        raise RuntimeError("rodent_amd: no GPU visible (torch.cuda.is_available() is False)")
    if bvh2.width != 2:
        raise ValueError("collapse_wide: a BVH2 / Tri1 hierarchy is needed")
    if width not in (4, 8):
        raise BuildError(f"collapse_wide: {_ERRORS[ERR_WIDTH]}")
    if not 0 <= stack_limit <= MAX_STACK_LIMIT:
        raise BuildError(f"collapse_wide: {_ERRORS[ERR_STACK_LIMIT]}")
    dev = bvh2.dev
    # without a limit the entry, its arguments and its scratch are what they were
    entry, limit, sizes = (("rodent_hip_collapse_bvh2_tri1_bounded", (int(stack_limit),), "rodent_hip_collapse_bounded_scratch_bytes")
                           if stack_limit else ("rodent_hip_collapse_bvh2_tri1", (), "rodent_hip_collapse_scratch_bytes"))
    need = getattr(abi.lib(), sizes)(width, bvh2.num_nodes, bvh2.num_tris)
    if need < 0:
        raise BuildError(f"{entry}: {_ERRORS[ERR_NUM_NODES]}")
    cuda = f"cuda:{dev}"
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty(need, dtype=torch.uint8, device=cuda)
    node_dt = {4: F.NODE4, 8: F.NODE8}[width]
    nodes = torch.empty(bvh2.num_nodes * node_dt.itemsize, dtype=torch.uint8, device=cuda)
    tris = torch.empty(bvh2.num_tris * F.TRI4.itemsize, dtype=torch.uint8, device=cuda)
    info = torch.empty(INFO_WORDS, dtype=torch.int32, device=cuda)
    words = _enqueue(entry, dev, stream, info, (bvh2.nodes, bvh2.tris, nodes, tris, scratch), int(width), *limit, bvh2.nodes.data_ptr(),
                     bvh2.num_nodes, bvh2.tris.data_ptr(), bvh2.num_tris, nodes.data_ptr(), tris.data_ptr(), scratch.data_ptr())
    _raise_flags(entry, words)
    wide = abi.DeviceBvh.from_tensors(width, nodes, tris, int(words[0]), int(words[1]), dev)
    wide.info, wide.scratch = words.copy(), scratch
    return wide


def build_wide(vertices, indices, width, dev=0, stream=None, stack_limit=0, **options) -> abi.DeviceBvh:
    """build_bvh2(vertices, indices, **options) then collapse_wide(..., width, stack_limit=stack_limit) on one stream: a BVH4 / BVH8 +
    Tri4 hierarchy built without the host builder.  The BVH2 it came from stays reachable as `.bvh2` (refit_wide needs only the wide
    tree)."""
    if width not in (4, 8):
        raise BuildError(f"build_wide: {_ERRORS[ERR_WIDTH]}")
    if not 0 <= stack_limit <= MAX_STACK_LIMIT:
        raise BuildError(f"build_wide: {_ERRORS[ERR_STACK_LIMIT]}")
    bvh2 = build_bvh2(vertices, indices, dev=dev, stream=stream, **options)
    wide = collapse_wide(bvh2, width, stream=stream, stack_limit=stack_limit)
    wide.bvh2 = bvh2
    return wide


def download_wide(bvh: abi.DeviceBvh):
    """(nodes, tris) host copies of a DeviceBvh of any width: NODE2 / TRI1, NODE4 / TRI4 or NODE8 / TRI4."""
    node_dt, tri_dt = {2: (F.NODE2, F.TRI1), 4: (F.NODE4, F.TRI4), 8: (F.NODE8, F.TRI4)}[bvh.width]
    nodes = bvh.nodes.view(torch.uint8)[: bvh.num_nodes * node_dt.itemsize].cpu().numpy().view(node_dt).copy()
    tris = bvh.tris.view(torch.uint8)[: bvh.num_tris * tri_dt.itemsize].cpu().numpy().view(tri_dt).copy()
    return nodes, tris


def download(bvh: abi.DeviceBvh):
    """(nodes NODE2, tris TRI1) host copies of a BVH2 / Tri1 DeviceBvh."""
    if bvh.width != 2:
        raise ValueError("download: a BVH2 / Tri1 hierarchy is needed (download_wide takes any width)")
    return download_wide(bvh)


def main(argv=None):
    from .scene import Scene
    ap = argparse.ArgumentParser(prog="python -m rodent_amd.gpubuild", description="BVH2 / Tri1 of a .rscene's mesh, built on the GPU")
    ap.add_argument("scene", help=".rscene file (converter)")
    ap.add_argument("-o", "--output", required=True, help=".bvh file to write (BVH2_TRI1 block)")
    ap.add_argument("--max-leaf", type=int, default=2, help="largest leaf (1 ... 8, default 2)")
    ap.add_argument("--treelet-passes", type=int, default=0,
                    help="treelet restructuring passes + SAH leaf collapse (0 ... 3, default 0: the LBVH as it is)")
    ap.add_argument("--split-budget", type=float, default=0.0,
                    help="pre-split triangles into up to this fraction of extra references (0 ... 4, default 0: no splitting)")
    ap.add_argument("--max-pieces", type=int, default=None, help="the most references one triangle may become (1 ... 64, default 64)")
    ap.add_argument("--ploc-radius", type=int, default=0,
                    help="topology by locally-ordered clustering over this many Morton neighbours to either side (1 ... 64, default 0: the "
                         "LBVH's)")
    ap.add_argument("--depth-limit", type=int, default=0, help="with --ploc-radius: the most Node2 levels (default 0: 56)")
    ap.add_argument("--width", type=int, action="append", choices=(4, 8), default=[],
                    help="also write the BVH2 collapsed into this width (BVH4_TRI4 / BVH8_TRI4 block); may be given twice")
    ap.add_argument("--stack-limit", type=int, default=0,
                    help="collapse under this stack limit: the stack bound is then at most max(L, the BVH2's own) (0 ... 63, default 0: none)")
    ap.add_argument("--dev", type=int, default=0)
    a = ap.parse_args(argv)
    sc = Scene(a.scene)
    bvh = build_bvh2(sc.vertices, sc.indices, a.max_leaf, a.dev, treelet_passes=a.treelet_passes, split_budget=a.split_budget,
                     max_pieces=a.max_pieces, ploc_radius=a.ploc_radius, depth_limit=a.depth_limit)
    nodes, tris = download(bvh)
    blocks = [(F.BVH2_TRI1, nodes, tris)]
    print(f"{a.output}: {len(tris)} triangles, {len(nodes)} nodes, depth {bvh.depth}")
    for width in sorted(set(a.width)):
        wide = collapse_wide(bvh, width, stack_limit=a.stack_limit)
        blocks.append((abi.BLOCK_OF_WIDTH[width], *download_wide(wide)))
        print(f"{a.output}: BVH{width}: {wide.num_nodes} nodes, {wide.num_tris} packets, stack bound {wide.info[3]}")
    F.write_bvh(a.output, blocks)


if __name__ == "__main__":
    main()
