/*
 * rodent_build.h -- C ABI of the device BVH builder (librodent_hip.so, rodent_amd/csrc/bvh_build.hip).
 *
 * A linear BVH (Morton codes + Karras 2012 hierarchy) built on the GPU from the renderer's own scene arrays
 * (RodentSceneDesc: float4 per vertex, int4 per triangle = v0 v1 v2 geometry id), written as BVH2 / Tri1 in the layout of
 * rodent_traversal.h, so every traversal and render entry point takes it as it is.
 *
 * Determinism: the output is a pure function of (vertices, indices, num_vertices, num_tris, max_leaf), byte for byte, whatever the
 * stream, the device load or the scratch contents; tests/lbvh_model.py restates every stage on the CPU and predicts the bytes.
 *
 * Layout of the result:
 *   - Node2 0 is the root; kept inner nodes (more than max_leaf triangles) are numbered in the order of their Karras index.
 *     child[0] is the left range, child[1] the right one: inner child = node index + 1, leaf = ~first triangle.
 *   - Tri1 k is the k-th triangle in (Morton code, triangle id) order: v0, e1 = v0 - v1, e2 = v2 - v0, geom_id = indices.w,
 *     prim_id = triangle id with bit 31 set on the last triangle of a leaf; the pad words are 0.
 *   - num_tris <= max_leaf: a single root whose child 0 is the whole leaf, child 1 = 0 with bounds (+inf, -inf).
 *   - The depth (Node2 levels on the longest path) is at most 30 + ceil(log2 num_tris): 55 at the size limit.
 */
#ifndef RODENT_BUILD_H
#define RODENT_BUILD_H

#include <stdint.h>
#include "rodent_traversal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RODENT_BUILD_MAX_TRIS    (1 << 25)
#define RODENT_BUILD_MAX_LEAF    8
#define RODENT_BUILD_INFO_WORDS  4      /* info: [0] Node2 count, [1] depth, [2] error flags (below), [3] 0 (optimising builder:
                                           topologies rejected by the depth rule) */

/* error flags in info[2] (found on the device; the hierarchy is then undefined, but nothing is read out of bounds) */
#define RODENT_BUILD_BAD_INDEX   1      /* a vertex index outside [0, num_vertices): that vertex is read as the origin */
#define RODENT_BUILD_NON_FINITE  2      /* a vertex coordinate is NaN or infinite */

/* return values (host-side checks: nothing is enqueued when they fail) */
#define RODENT_BUILD_OK                 0
#define RODENT_BUILD_ERR_NUM_TRIS      -1   /* num_tris outside [1, 2^25] */
#define RODENT_BUILD_ERR_MAX_LEAF      -2   /* max_leaf outside [1, 8] */
#define RODENT_BUILD_ERR_NUM_VERTICES  -3   /* num_vertices < 1 */
#define RODENT_BUILD_ERR_NULL          -4   /* a NULL pointer */
#define RODENT_BUILD_ERR_DEVICE        -5   /* no such device */
#define RODENT_BUILD_ERR_LAUNCH        -6   /* the HIP runtime refused a launch / an allocation (sync form) */
#define RODENT_BUILD_ERR_INPUT         -7   /* sync form only: the device raised an error flag (info[2]) */
#define RODENT_BUILD_ERR_PASSES        -8   /* RodentBuildOptions.treelet_passes outside [0, 3] */
#define RODENT_BUILD_ERR_COST          -9   /* RodentBuildOptions.node_cost / tri_cost not in (0, 1e6] */

/* Bytes of device scratch rodent_hip_build_bvh2_tri1 needs for num_tris triangles (-1 outside [1, 2^25]); any 256-byte aligned
 * buffer of that size, its contents are ignored. */
int64_t rodent_hip_build_scratch_bytes(int32_t num_tris);

/* Builds the hierarchy of num_tris triangles.  All pointers are DEVICE pointers: vertices (4 floats per vertex), indices
 * (4 ints per triangle), nodes (room for max(1, num_tris - 1) Node2), tris (num_tris Tri1), scratch
 * (rodent_hip_build_scratch_bytes), info_dev (RODENT_BUILD_INFO_WORDS ints).  Asynchronous: everything is enqueued on `stream`
 * (a hipStream_t, NULL = the null stream); nothing is allocated and nothing waits for the device.  info_dev is zeroed at the
 * start of the call and holds the node count, depth and error flags once the stream reaches the end of it.  max_leaf: the
 * largest leaf (2 is the host SBVH builder's leaf threshold).  Returns RODENT_BUILD_OK or one of the errors above. */
int32_t rodent_hip_build_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev,
                                   void* stream);

/* Synchronous form on the null stream: allocates and frees its own scratch, copies the RODENT_BUILD_INFO_WORDS info words to
 * `info` (host, may be NULL) and returns RODENT_BUILD_ERR_INPUT when the device raised a flag. */
int32_t rodent_hip_build_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, int32_t* info);

/* ---- the optimising builder: treelet restructuring + SAH leaf collapse ------------------------------------------------------
 *
 * After the LBVH's Karras tree (single-triangle leaves), `treelet_passes` passes of treelet restructuring (Karras & Aila, "Fast
 * Parallel Construction of High-Quality Bounding Volume Hierarchies", HPG 2013) and a surface-area (SAH) leaf collapse.  The output
 * is a pure function of (vertices, indices, num_vertices, num_tris, options), byte for byte; tests/trbvh_model.py restates every stage.
 *
 * Costs, all fp32 in this order (A = half the surface area of a box, (dx * dy + dy * dz) + dz * dx; N = triangles under a node):
 *   C(triangle) = (tri_cost * A) * 1;   inner = node_cost * A + (C(left) + C(right));   leaf = (tri_cost * A) * N
 *   C(node) = leaf when N <= max_leaf and leaf <= inner, else inner: such a node is COLLAPSED.
 * Passes: pass k (0-based) visits the nodes bottom-up and restructures the treelet of every node with at least gamma_k = 7 << k
 *   triangles (7, 14, 28):
 *   - growth: the treelet's leaves start as the node's two children; five times, the leaf of largest A that is an inner node (ties:
 *     the lowest slot) is replaced by its left child and its right child takes the next slot: 7 leaves, 6 inner nodes.
 *   - DP over the 127 non-empty subsets S of the 7 leaves by size: the best split of S is the first P, among the subsets of S that
 *     hold S's lowest leaf (S itself excluded) in increasing bit order, of least C(P) + C(S \ P); C(S) as above, with that sum.
 *   - depth rule: with d(n) the inner nodes above n at the start of the pass, the new topology is taken only when its height
 *     (Node2 levels, single-triangle leaves, computed from the slots' stored heights) is at most 56 - d(n); otherwise the treelet
 *     stays as it is and only the node's height and cost are refitted from its current children, so every stored height is true
 *     when an ancestor reads it.  A pass never lengthens the path above a node it visits, so by induction every tree has at most
 *     56 levels (the LBVH's Karras tree has at most 55), and
 *     the collapse only shortens it.  info[3] counts the rejected topologies over all passes.
 *   - the new inner nodes, in pre-order (the part holding the lowest leaf first), take the node's own id, then the ids of the
 *     expanded nodes in expansion order; the node keeps its id, so the links above it stay valid.
 * Collapse and emission: a node is a leaf when it is collapsed and no ancestor is; the root too (then the single-leaf form above).
 *   Node2 records in depth-first pre-order, child 0 first (root 0, an inner child 0 at index + 1); Tri1 records in the leaves'
 *   left-to-right order; prim_id and the end-of-leaf bit as above.  info[0] and info[1] as above; max_leaf is an upper bound on a
 *   leaf, not a threshold.  treelet_passes = 0 gives exactly the bytes of rodent_hip_build_bvh2_tri1 with the same max_leaf. */
#define RODENT_BUILD_MAX_TREELET_PASSES  3
#define RODENT_BUILD_DEFAULT_NODE_COST   1.2f    /* Karras & Aila's C_i */
#define RODENT_BUILD_DEFAULT_TRI_COST    1.0f    /* Karras & Aila's C_t */

struct RodentBuildOptions {
    int32_t max_leaf;          /* 1 ... 8: the largest leaf */
    int32_t treelet_passes;    /* 0 ... 3: 0 = the LBVH of rodent_hip_build_bvh2_tri1 */
    float node_cost, tri_cost; /* SAH cost of a node visit and of a triangle test, in (0, 1e6] (defaults above) */
};

/* Bytes of device scratch rodent_hip_build_bvh2_tri1_opt needs (-1 for num_tris outside [1, 2^25] or invalid options). */
int64_t rodent_hip_build_opt_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt);

/* rodent_hip_build_bvh2_tri1 with options: the same arguments, buffers and node buffer size (max(1, num_tris - 1) Node2), scratch of
 * rodent_hip_build_opt_scratch_bytes.  Invalid options (NULL: RODENT_BUILD_ERR_NULL, RODENT_BUILD_ERR_MAX_LEAF / _PASSES / _COST)
 * are refused before anything is enqueued. */
int32_t rodent_hip_build_bvh2_tri1_opt(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                       int32_t num_tris, const struct RodentBuildOptions* opt, struct Node2* nodes, struct Tri1* tris,
                                       void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form, as rodent_hip_build_bvh2_tri1_sync. */
int32_t rodent_hip_build_bvh2_tri1_opt_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                            int32_t num_tris, const struct RodentBuildOptions* opt, struct Node2* nodes,
                                            struct Tri1* tris, int32_t* info);

/* ---- triangle pre-splitting (Karras & Aila, HPG 2013, section 5) ----------------------------------------------------------------
 *
 * Before the Morton codes, the triangles whose boxes waste the most area are cut along planes of a grid into several REFERENCES,
 * each with a tighter box; the stages above (the LBVH for treelet_passes = 0, the optimising builder otherwise) then run over the
 * n' references instead of the n triangles.  A Tri1 record holds the whole triangle and its id, so a triangle may appear in several
 * leaves (or twice in one).  The output is a pure function of (vertices, indices, num_vertices, num_tris, options, split options),
 * byte for byte; tests/split_model.py restates every stage.  All arithmetic is fp32 in the order written (only + - * and correctly
 * rounded division and square root), integer sums, exact min / max.  Vertex coordinates are taken as x + 0 (no -0).
 *
 * Frame: the union of the triangle boxes, lo_a ... hi_a per axis; step_a = (hi_a - lo_a) * 0x1p-10f when that is finite and > 0,
 *   otherwise the axis has no planes.  Plane c (1 ... 1023) of axis a lies at lo_a + (float)c * step_a; its level is ctz(c) (9 the
 *   coarsest).  The plane of a box: the coarsest plane lying strictly inside the box on its axis (lo < plane < hi), ties to x, y, z.
 * Priority of triangle t (box b, n = (v1 - v0) x (v2 - v0) component by component, x = ey * fz - ez * fy, and so on):
 *   excess = max(0, A(b) - 0.5f * ((|nx| + |ny|) + |nz|)),  p = sqrt(2^L * excess), L the level of b's plane; p = 0 when b has no
 *   plane, when the triangle raised an error flag, and when p is not finite (Karras & Aila's exponent 1/3 becomes a square root).
 * Allotment, B = min(floor(budget * n) (exact product), 2^25 - n) extra references:
 *   pmax = max p;  w = (uint32)floorf(__fdiv_rn(p, pmax) * 65536.0f) (0 when pmax = 0);  W = sum of w (uint64);
 *   s = min(max_pieces - 1, (w * B) / W) in 64-bit integers (0 when W = 0): the triangle may become s + 1 pieces, sum s <= B.
 * Cutting (triangles with s > 0; a piece is a box and a count k of splits it still holds; the first piece is the triangle's box, k = s):
 *   loop: k = 0, or the piece's box has no plane -> the piece is final (its k splits are "not made", counted in info[6]);
 *   otherwise cut at the plane (axis a, position x): each vertex goes to the side(s) it lies on (v_a <= x left, v_a >= x right); each
 *   edge v_i -> v_{i+1 mod 3} with its ends strictly on opposite sides adds, to both sides, the point of axis-a coordinate x and, on
 *   each other axis b, the interval [max(y - g, min(p_b, q_b)), min(y + g, max(p_b, q_b))], with t = __fdiv_rn(x - p_a, q_a - p_a),
 *   y = p_b + t * (q_b - p_b) and the margin g = max(max(|p_b|, |q_b|) * 0x1p-19f, 0x1p-126f), which exceeds the rounding error of
 *   y (about 12 ulps of max(|p_b|, |q_b|)); a side's box, the box of its points, is then intersected with the piece's box and
 *   clamped to its half space.  When one side's box is empty the piece takes the other side's box and keeps its k (the plane then
 *   lies on its border, so this ends); when both are, the piece is final with its k not made.  Otherwise the left side gets
 *   kl = (int)min(max(floorf(__fdiv_rn((float)(k - 1) * el, el + er) + 0.5f), 0), k - 1) splits (a NaN quotient gives 0), the right
 *   side k - 1 - kl; el, er are the sides' longest extents.  Pieces are final in depth-first order, left side first.
 * References: every triangle's pieces in that order, triangles in id order (an exclusive scan).  An uncut triangle's box is its
 *   triangle box and its Morton point the vertex sum (v0 + v1) + v2; a piece's point is (lo + hi) * 1.5f per axis (the same 3x scale).
 *   The stages above then run over the references: the Morton frame is the bounds of the references' points, the sort orders
 *   (code, reference index), leaf boxes are the references' boxes and Tri1 records their triangles.  n' <= 2^25, so the depth bounds
 *   above (55 for the LBVH, 56 with treelets) hold.  budget = 0 or max_pieces = 1: the bytes of rodent_hip_build_bvh2_tri1_opt. */
#define RODENT_BUILD_SPLIT_INFO_WORDS  8   /* [0] Node2 count [1] depth [2] flags [3] rejected topologies
                                              [4] Tri1 count (references) [5] triangles split [6] splits allotted but not made [7] 0 */
#define RODENT_BUILD_MAX_PIECES        64
#define RODENT_BUILD_MAX_SPLIT_BUDGET  4.0f
#define RODENT_BUILD_ERR_SPLIT        -10  /* RodentSplitOptions out of range */

struct RodentSplitOptions {
    float   budget;      /* [0, 4]: extra references as a fraction of num_tris; 0 = no splitting */
    int32_t max_pieces;  /* 1 ... 64: the most references one triangle may become */
};

/* The most references the split builder can make: num_tris + min(B, num_tris * (max_pieces - 1)) (-1 on invalid arguments).  The
 * node buffer holds max(1, max_refs - 1) Node2, the triangle buffer max_refs Tri1. */
int64_t rodent_hip_build_split_max_refs(int32_t num_tris, const struct RodentSplitOptions* split);

/* Bytes of device scratch rodent_hip_build_bvh2_tri1_split needs (-1 on invalid arguments). */
int64_t rodent_hip_build_split_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt,
                                             const struct RodentSplitOptions* split);

/* rodent_hip_build_bvh2_tri1_opt over pre-split references: the same arguments plus `split`; nodes: max(1, max_refs - 1) Node2,
 * tris: max_refs Tri1, info_dev: RODENT_BUILD_SPLIT_INFO_WORDS ints (info[4] = the Tri1 count).  Asynchronous like the others:
 * nothing is allocated, nothing waits for the device.  Invalid split options: RODENT_BUILD_ERR_SPLIT before anything is enqueued. */
int32_t rodent_hip_build_bvh2_tri1_split(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                         int32_t num_tris, const struct RodentBuildOptions* opt, const struct RodentSplitOptions* split,
                                         struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form, as rodent_hip_build_bvh2_tri1_opt_sync; `info` receives RODENT_BUILD_SPLIT_INFO_WORDS words. */
int32_t rodent_hip_build_bvh2_tri1_split_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                              int32_t num_tris, const struct RodentBuildOptions* opt,
                                              const struct RodentSplitOptions* split, struct Node2* nodes, struct Tri1* tris,
                                              int32_t* info);

/* ---- topology by parallel locally-ordered clustering, PLOC (Meister & Bittner, "Parallel Locally-Ordered Clustering for Bounding
 * Volume Hierarchy Construction", TVCG 2018) ---------------------------------------------------------------------------------------------
 *
 * Another way to choose the topology: instead of Karras' hierarchy over the Morton codes, the references, lying in (Morton code,
 * reference index) order, are merged bottom-up, each with the neighbour whose union with it is smallest.  Everything before (the split
 * front, the codes, the sort, the Tri1 records in sorted order) and after (fit, treelet passes, SAH leaf collapse, pre-order emission: the
 * optimising builder above, treelet_passes = 0 allowed and meaning clustering + collapse) is as it stands.  The output is a pure function
 * of (vertices, indices, num_vertices, num_tris, options, split options, PLOC options radius and depth_limit), byte for byte;
 * tests/ploc_model.py restates the rule.  wide_iterations is scheduling only and changes no byte.
 *
 * Ids: with n references (n' of the split front) and m = n - 1: 0 ... m-1 inner nodes, m + p the sorted reference p.
 * Cluster: an id, a box and a height h; a reference has h = 0, a merge h = 1 + max of its two parts.  At the start the clusters are the
 *   references in sorted order.  C: the clusters at the start of iteration t = 0, 1, ...; clog2(x) = ceil(log2 x), clog2(1) = 0;
 *   D = depth_limit (0 means 56);  I = 4 * clog2(n) + 8.
 * Nearest-neighbour iteration (t < I): the candidates of the cluster at position i are the positions j != i with |i - j| <= radius that
 *   are admissible: 1 + max(h_i, h_j) <= D - clog2(C).  d(i, j) = A of the exact union of the two boxes (min of the lows, max of the highs;
 *   A as above, fp32 in that order); a NaN d is never chosen.  i chooses the candidate of least d, equal d going to the smaller i ^ j
 *   (for a fixed i, j -> i ^ j is injective: the choice is unique; the key (d, i ^ j) is symmetric, so the pair of least key among all
 *   has chosen each other: while any candidate pair exists, an iteration merges; identical boxes pair up as (0,1), (2,3), ... and do not
 *   form a chain).  Without a candidate i chooses nobody.  i and j merge when each chose the other.
 * Forced iteration (t >= I): positions 2k and 2k + 1 merge whatever their boxes; a last odd position stays.
 * Merging, in either kind: the lower position leads; left = the leader's id, right = the partner's; the new node's id =
 *   (C - 2) - (leaders at lower positions in this iteration), so C - 1 merges are left for ids C - 2 ... 0 and the last merge is node 0,
 *   the root the tail's walks start from; parent links of both parts are written, the root's is -1.  The merged cluster takes the
 *   leader's position, the partner's slot is dropped, the others keep their order.  Iterations run until C = 1; n = 1: no iteration, the
 *   single-leaf root as everywhere.
 * Depth: every height is at most D - clog2(C) at the start of every iteration.  At t = 0: h = 0 and D >= clog2(n) (checked by the
 *   entry).  A nearest-neighbour iteration only makes admissible merges, 1 + max(h_i, h_j) <= D - clog2(C), and the next C is no larger,
 *   so D - clog2(C) does not fall.  A forced iteration turns C >= 2 clusters into ceil(C / 2), and clog2(ceil(C / 2)) = clog2(C) - 1,
 *   while a height grows by one at most.  At C = 1 the root's height, the Node2 levels of the tree, is therefore at most D; the leaf
 *   collapse only shortens paths.  The treelet passes' own rule is tied to 56 levels, so D < 56 with treelet_passes > 0 is refused.
 * Iterations: at most I nearest-neighbour ones, then every iteration halves C: at most I + clog2(n) <= 4 * 25 + 8 + 25 = 133.
 * info: the split entry's 8 words; [4] the Tri1 count (num_tris without split options), [5], [6] as there (0 without), [7] the
 *   iterations run until one cluster was left; forced ones ran exactly when [7] > I. */
#define RODENT_BUILD_MAX_PLOC_RADIUS   64
#define RODENT_BUILD_MAX_DEPTH         56
#define RODENT_BUILD_ERR_PLOC         -16  /* RodentPlocOptions out of range, depth_limit below clog2(the most references), or
                                              depth_limit < 56 together with treelet passes */

struct RodentPlocOptions {
    int32_t radius;           /* 1 ... 64: positions searched to either side */
    int32_t depth_limit;      /* 0 ... 56: the most Node2 levels, 0 = 56; at least clog2(the most references) */
    int32_t wide_iterations;  /* -1 ... 255: device-wide iterations before one workgroup finishes the clustering; -1 = the library's
                                 choice.  Scheduling only: the output does not depend on it */
};

/* Bytes of device scratch rodent_hip_build_bvh2_tri1_ploc needs (-1 on invalid arguments).  split may be NULL: no pre-splitting. */
int64_t rodent_hip_build_ploc_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt,
                                            const struct RodentSplitOptions* split, const struct RodentPlocOptions* ploc);

/* rodent_hip_build_bvh2_tri1_split with the PLOC topology stage.  split may be NULL (no pre-splitting: nodes hold max(1, num_tris - 1)
 * Node2, tris num_tris Tri1); with it the buffer sizes come from rodent_hip_build_split_max_refs.  info_dev:
 * RODENT_BUILD_SPLIT_INFO_WORDS ints either way.  Asynchronous like the others: a fixed list of launches on `stream` that depends on
 * num_tris and the options alone, nothing allocated, nothing waits for the device or for another workgroup.  Checks, in this order,
 * each enqueuing nothing when it fails: the options' (as the split entry, split's only when it is given), ploc NULL
 * (RODENT_BUILD_ERR_NULL), RODENT_BUILD_ERR_PLOC (its depth_limit against the reference count only when num_tris is in range), then
 * the mesh arguments'. */
int32_t rodent_hip_build_bvh2_tri1_ploc(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, const struct RodentBuildOptions* opt, const struct RodentSplitOptions* split,
                                        const struct RodentPlocOptions* ploc, struct Node2* nodes, struct Tri1* tris, void* scratch,
                                        int32_t* info_dev, void* stream);

/* Synchronous form, as rodent_hip_build_bvh2_tri1_split_sync. */
int32_t rodent_hip_build_bvh2_tri1_ploc_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                             int32_t num_tris, const struct RodentBuildOptions* opt,
                                             const struct RodentSplitOptions* split, const struct RodentPlocOptions* ploc,
                                             struct Node2* nodes, struct Tri1* tris, int32_t* info);

/* ---- refit: new boxes and Tri1 records for an existing hierarchy whose vertices moved ------------------------------------------------
 *
 * The topology stays: the child, pad and w words (pad, geom_id, prim_id with its end-of-leaf bit) are read and never written; only the
 * 12 bounds of a Node2 and v0 / e1 / e2 of a Tri1 are.  No sort, no hierarchy search, no emission: three launches.  The hierarchy may
 * come from any of the builders above or from a host builder (any BVH2 / Tri1 of rodent_traversal.h whose records name their
 * triangles by prim_id & 0x7FFFFFFF); builder scratch is not looked at.  The result is a pure function of (nodes, tris, vertices,
 * indices), byte for byte (fp32, exact min / max, which do not depend on the order they are taken in); tests/refit_model.py restates it.
 *
 * Tri1 record p, t = prim_id & 0x7FFFFFFF: the corners are read as the builders read them (an index outside [0, num_vertices) reads
 *   as the origin and raises RODENT_BUILD_BAD_INDEX, a non-finite coordinate raises RODENT_BUILD_NON_FINITE); v0, e1 = v0 - v1,
 *   e2 = v2 - v0 by the builders' own statements.  t >= num_tris raises RODENT_BUILD_BAD_TOPOLOGY: the record stays as it is and its
 *   box is empty.  The box of a record: per axis the min and max of c + 0 over the three corners.
 * Child slot k of node i: child == 0: the 6 bounds stay as stored.  child < 0: the union of the boxes of records ~child, ~child + 1, ...
 *   up to and including the first with the end-of-leaf bit; a walk that reaches num_bvh_tris without one raises the flag and leaves the
 *   slot as stored.  child > 0: the union of the two boxes of node child - 1 (min of the lows, max of the highs; an empty slot's
 *   (+inf, -inf) drops out by itself).
 * Malformed trees: a child id > num_nodes, the root as a child (id 1), a leaf start >= num_bvh_tris and a node named by two slots (the
 *   second one found) raise RODENT_BUILD_BAD_TOPOLOGY; such a slot stays as stored, and a node with such an inner slot, and every node
 *   above it, is not completed: info[0] < num_nodes.  Nothing is read out of bounds and every walk is bounded (a leaf by num_bvh_tris;
 *   a node is completed at most once, so the climb by num_nodes).
 * info: [0] nodes completed (num_nodes for a sound tree) [1] Tri1 records rewritten [2] flags [3] 0.
 *
 * Identity: a hierarchy written by rodent_hip_build_bvh2_tri1 or _opt, refitted with the vertices it was built from, keeps its bytes:
 *   those builders' boxes are exact unions of the same triangle boxes.
 * Split trees: rodent_hip_build_bvh2_tri1_split stores CLIPPED reference boxes; after a refit every reference carries its whole
 *   triangle's box, which contains the clipped one: correct and conservative, but looser, so a split tree refitted with its own vertices
 *   is not byte-identical, and every refitted box contains the box it replaces. */
#define RODENT_BUILD_BAD_TOPOLOGY      4    /* info[2], refit: a child id out of range, a leaf without an end bit, a prim_id outside the
                                               index array, a node claimed by two parents */
#define RODENT_BUILD_ERR_NUM_NODES   -11    /* num_nodes < 1 or num_bvh_tris < 1 */

/* Bytes of device scratch rodent_hip_refit_bvh2_tri1 needs (-1 when num_nodes < 1 or num_bvh_tris < 1). */
int64_t rodent_hip_refit_scratch_bytes(int32_t num_nodes, int32_t num_bvh_tris);

/* Refits nodes[num_nodes] / tris[num_bvh_tris] in place from vertices (num_vertices x 4 floats) and indices (num_tris x 4 ints).  All
 * pointers are DEVICE pointers; scratch: rodent_hip_refit_scratch_bytes, contents ignored; info_dev: RODENT_BUILD_INFO_WORDS ints,
 * zeroed at the start of the call.  Asynchronous on `stream` like the builders: nothing is allocated, nothing waits for the device.
 * The argument checks and return values are the builders'; a failed check enqueues nothing. */
int32_t rodent_hip_refit_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node2* nodes, int32_t num_nodes, struct Tri1* tris, int32_t num_bvh_tris, void* scratch,
                                   int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch; RODENT_BUILD_ERR_INPUT when a flag is raised or info[0] != num_nodes. */
int32_t rodent_hip_refit_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node2* nodes, int32_t num_nodes, struct Tri1* tris,
                                        int32_t num_bvh_tris, int32_t* info);

/* ---- refit of the wide layouts: Node4 / Node8 + Tri4 ------------------------------------------------------------------------------------
 *
 * The BVH2 refit above for the hierarchies of hip_traverse_bvh4_tri4_async / _bvh8_tri4_async (N = 4 or 8 slots to a node, Tri4 packets
 * of four lanes).  Any tree of the layout, from any builder; three launches, no builder scratch.  tests/refit_wide_model.py restates it.
 *
 * Touched: the topology stays: child, pad, every prim_id and every geom_id are read and never written.  Written: the 6 x N bounds of a
 *   node, and columns v0, e1, e2, n of the VALID lanes of a Tri4.  Lanes that are not valid keep their stored bytes (the host builder
 *   leaves them 0).
 * Valid lanes: lane k of a packet is valid when none of prim_id[0 .. k] equals -1 (the traversal kernels' rule: == -1 ends the packet);
 *   its triangle is t = prim_id[k] & 0x7FFFFFFF.  A packet ends its leaf when prim_id[3] < 0.
 * A valid lane, t < num_tris: the corners are read as the builders read them (an index outside [0, num_vertices) reads as the origin
 *   and raises RODENT_BUILD_BAD_INDEX, a non-finite coordinate raises RODENT_BUILD_NON_FINITE); v0, e1 = v0 - v1, e2 = v2 - v0 by the
 *   builders' own statements; n = e1 x e2 component by component as the host builder's cross: nx = e1y * e2z - e1z * e2y,
 *   ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x, each product rounded on its own (no fused multiply-add).  Its box: per axis
 *   the min and max of c + 0 over the three corners.
 * A valid lane, t >= num_tris: raises RODENT_BUILD_BAD_TOPOLOGY; the lane stays as stored and its box is empty.
 * A packet's box: the union of its valid lanes' boxes; (+inf, -inf) when it has none.
 * Slot k of node i: child == 0: the six bounds stay as stored.  child < 0: the union of the boxes of packets ~child, ~child + 1, ... up to
 *   and including the first that ends its leaf; a start >= num_packets, and a walk that reaches num_packets without an end, raise the
 *   flag and leave the slot as stored.  child > 0: the union of all N slot boxes of node child - 1 (an empty slot's (+inf, -inf) drops
 *   out by itself).
 * Malformed trees: as for BVH2: a child id > num_nodes, the root as a child (id 1) and a node named by two slots (the second one found)
 *   raise RODENT_BUILD_BAD_TOPOLOGY; such a slot stays as stored, and a node with such an inner slot, and every node above it, is not
 *   completed: info[0] < num_nodes.  Nothing is read out of bounds and every walk is bounded (a leaf by num_packets, the climb by
 *   num_nodes).
 * info: [0] nodes completed (num_nodes for a sound tree) [1] lanes rewritten [2] flags [3] 0.
 * Determinism: the result is a pure function of (nodes, packets, vertices, indices), byte for byte.
 *
 * Identity: a tree of the host builder refitted with the vertices it was built from keeps its Tri4 bytes; every refitted box contains
 *   the stored one (the host builder's leaf boxes may be clipped by its spatial splits, and are then tighter than the triangles'). */

/* Bytes of device scratch rodent_hip_refit_bvh4_tri4 (width 4) / _bvh8_tri4 (width 8) needs; -1 for another width and when
 * num_nodes < 1 or num_packets < 1. */
int64_t rodent_hip_refit_wide_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_packets);

/* Refits nodes[num_nodes] / tris[num_packets] in place.  Arguments, checks, return values and asynchrony are those of
 * rodent_hip_refit_bvh2_tri1 (RODENT_BUILD_ERR_NUM_NODES: num_nodes < 1 or num_packets < 1); a failed check enqueues nothing. */
int32_t rodent_hip_refit_bvh4_tri4(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node4* nodes, int32_t num_nodes, struct Tri4* tris, int32_t num_packets, void* scratch,
                                   int32_t* info_dev, void* stream);
int32_t rodent_hip_refit_bvh8_tri4(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node8* nodes, int32_t num_nodes, struct Tri4* tris, int32_t num_packets, void* scratch,
                                   int32_t* info_dev, void* stream);

/* Synchronous forms, as rodent_hip_refit_bvh2_tri1_sync. */
int32_t rodent_hip_refit_bvh4_tri4_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node4* nodes, int32_t num_nodes, struct Tri4* tris,
                                        int32_t num_packets, int32_t* info);
int32_t rodent_hip_refit_bvh8_tri4_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node8* nodes, int32_t num_nodes, struct Tri4* tris,
                                        int32_t num_packets, int32_t* info);

/* ---- collapse into the wide layouts: BVH2 / Tri1 -> Node4 / Node8 + Tri4 ----------------------------------------------------------------
 *
 * Any BVH2 / Tri1 of rodent_traversal.h (of the builders above or of a host builder) becomes a hierarchy of N = 4 or 8 slots to a node
 * with Tri4 packets, as hip_traverse_bvh4_tri4_async / _bvh8_tri4_async and the wide refit take it.  No vertices: every word written is
 * a bit copy or an exact function of the Node2 and Tri1 records, so the result is a pure function of (N, nodes, tris), byte for byte;
 * tests/collapse_model.py restates it.  A fixed list of launches whatever the tree; no thread waits for another.
 *
 * Runs: a run is the records from a leaf start (~child) up to and including the first with the end-of-leaf bit.
 * Small subtrees: walk an inner node's subtree left to right (child 0 before child 1, child == 0 skipped).  It is SMALL when its runs
 *   hold at most 4 records in all and each run starts at the record after the previous run's last.  (It then has at most 3 inner nodes:
 *   the walk stops at the 5th record or the 4th inner node.)
 * Packet leaves: a child reference is a packet leaf when it is a BVH2 leaf (child < 0) or a small inner node; the topmost packet leaf
 *   on a path counts.  Its records are its runs in that order.  A small subtree makes exactly one Tri4 packet, a plain run of k
 *   records ceil(k / 4) packets (4 records each, the rest in the last).
 * Slots of the wide node rooted at BVH2 node r: r's children that are not 0, in order, each with the 6 bounds r stores for it.  While
 *   there are fewer than N slots: the candidates are the slots holding an inner node that is not small; A = (dx * dy + dy * dz) + dz * dx
 *   in fp32, every operation rounded on its own, d = hi - lo of the slot's stored bounds; the slots are scanned in order with
 *   best = -1 and a strict >, so the first of equals wins and a NaN never does; when none wins the growth stops.  The winning slot takes
 *   that node's child 0, that node's child 1 becomes the next slot, each with the bounds stored in the expanded node (the treelet growth
 *   rule above).  Slots keep this order.  Every slot that still holds an inner node which is not small is a wide root; the root of the
 *   tree is node 0.
 * Whole tree small (node 0 is small; the single-leaf form child[1] == 0 with at most 4 records too): one wide node whose slot 0 is the
 *   leaf over the union of node 0's two stored slot boxes (the (+inf, -inf) of an empty slot drops out by itself).
 * Numbering: wide nodes by ascending BVH2 index of their root (node 0 becomes wide node 0), packets by ascending first record: a
 *   pre-order BVH2 gives a pre-order wide tree.
 * Node record: column j of bounds is a bit copy of slot j's 6 stored bounds; child = wide id + 1 for an inner slot, ~first packet for
 *   a leaf slot; unused slots: child 0, bounds (+inf, -inf), as the host builder writes them; pad = 0.
 * Packet: lane j takes v0 / e1 / e2 of its record bit for bit; n = e1 x e2 component by component, every product rounded on its own
 *   (the wide refit's statement); prim_id = the record's prim_id & 0x7FFFFFFF, geom_id copied.  Unused lanes: prim_id -1, every other
 *   word 0.  The last packet of a leaf has bit 31 of prim_id[3] set (a -1 there has it already).
 * info: [0] wide nodes [1] packets [2] flags [3] the stack bound B: the maximum over the wide nodes of the sum, over the node and its
 *   ancestors, of (filled slots - 1).  A ray's traversal stack never holds more than B real entries, so B <= 63 guarantees that no ray
 *   overflows the kernels' 64 entries; above that nothing is guaranteed, exactly as for a host builder's tree.  B is information for
 *   the caller, not an error.
 * Stack limit (the _bounded entries; stack_limit L in [0, 63], L = 0: none, the collapse above byte for byte and launch for launch):
 *   Open: a child reference is open when it names a sound inner node that is not small: the candidates of the growth above.
 *   Height: for an inner node i that is not small, H(i) = 1 + max(h(child 0), h(child 1)), where h(ref) = H(ref - 1) when ref is open
 *     and 0 otherwise (leaves, small nodes and empty slots count 0).  H(i) is the stack bound of i's subtree left binary; no collapse
 *     of that subtree has a smaller one.  H is at most the number of nodes on the longest path: at most the builders' info[1] (<= 56)
 *     for a tree of this library.
 *   Growth: a wide node rooted at r is entered with S, the sum of (filled slots - 1) over its ancestors.  It starts with r's children
 *     as above.  While it has f < N slots, the candidates are the candidates above that also satisfy: for every OTHER filled slot s,
 *     S + f + h(s) <= L (f counted before the expansion).  The slot of largest A among them is expanded as above (the first of equals,
 *     never a NaN); growth stops when no candidate is left.
 *   Guarantee: B <= max(L, H(0)).  So L = 63 gives B <= 63 for every tree the builders above produce; for a deeper host tree
 *     info[3] > L says that the bound could not be met (then info[3] = H(0)).  B stays information, not an error.  When L is at least
 *     the B of the collapse without a limit, the result equals that collapse byte for byte.
 *   Everything else is as above: small subtrees, packets, numbering, bit-copied bounds, n, unused slots, flags, the malformed-tree
 *     list and the whole-tree-small form.  tests/collapse_bounded_model.py restates it.  One launch more (the heights).
 * Malformed trees raise RODENT_BUILD_BAD_TOPOLOGY; the output is then undefined, but nothing is read or written out of bounds and every
 *   loop keeps its bound: a child id > num_nodes, the root as a child (id 1), a node named by two slots, a node that does not reach
 *   the root within 64 parents, a leaf start >= num_bvh_tris, a leaf start whose predecessor has no end-of-leaf bit, a run longer than
 *   64 records, a run that reaches num_bvh_tris without an end bit; also a record held by two leaves, and an empty slot (child == 0) in
 *   a node other than the root or in both of the root's.
 *
 * Identity: a collapsed tree of an unsplit device build, refitted by rodent_hip_refit_bvh4_tri4 / _bvh8_tri4 with the vertices it was
 *   built from, keeps every byte: its slot boxes are bit copies of exact unions, and n is computed by the refit's own rule. */
#define RODENT_BUILD_ERR_WIDTH       -12    /* width other than 4 or 8 */
#define RODENT_BUILD_ERR_STACK_LIMIT -13    /* stack_limit outside [0, 63] */
#define RODENT_BUILD_MAX_STACK_LIMIT 63

/* Bytes of device scratch rodent_hip_collapse_bvh2_tri1 needs; -1 for a width other than 4 or 8 and when num_nodes < 1 or
 * num_bvh_tris < 1. */
int64_t rodent_hip_collapse_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_bvh_tris);

/* Collapses nodes[num_nodes] / tris[num_bvh_tris] into wide_nodes (room for num_nodes Node4 when width = 4, Node8 when width = 8) and
 * packets (room for num_bvh_tris Tri4).  All pointers are DEVICE pointers; the input is only read; scratch:
 * rodent_hip_collapse_scratch_bytes, contents ignored; info_dev: RODENT_BUILD_INFO_WORDS ints, zeroed at the start of the call.
 * Asynchronous on `stream` like the builders: nothing is allocated, nothing waits for the device.  Checks, in this order, each enqueuing
 * nothing when it fails: RODENT_BUILD_ERR_WIDTH, then the refit's RODENT_BUILD_ERR_NUM_NODES, _NULL and _DEVICE. */
int32_t rodent_hip_collapse_bvh2_tri1(int32_t dev, int32_t width, const struct Node2* nodes, int32_t num_nodes, const struct Tri1* tris,
                                      int32_t num_bvh_tris, void* wide_nodes, struct Tri4* packets, void* scratch, int32_t* info_dev,
                                      void* stream);

/* Synchronous form on the null stream with its own scratch; RODENT_BUILD_ERR_INPUT when the device raised a flag. */
int32_t rodent_hip_collapse_bvh2_tri1_sync(int32_t dev, int32_t width, const struct Node2* nodes, int32_t num_nodes,
                                           const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes, struct Tri4* packets,
                                           int32_t* info);

/* Bytes of device scratch rodent_hip_collapse_bvh2_tri1_bounded needs (two ints per node more than
 * rodent_hip_collapse_scratch_bytes, whatever stack_limit); -1 as there. */
int64_t rodent_hip_collapse_bounded_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_bvh_tris);

/* rodent_hip_collapse_bvh2_tri1 with a stack limit (rules above; 0: none, the same bytes, info words and launches as that entry).
 * scratch: rodent_hip_collapse_bounded_scratch_bytes.  Checks, in this order, each enqueuing nothing when it fails:
 * RODENT_BUILD_ERR_WIDTH, RODENT_BUILD_ERR_STACK_LIMIT, then RODENT_BUILD_ERR_NUM_NODES, _NULL and _DEVICE. */
int32_t rodent_hip_collapse_bvh2_tri1_bounded(int32_t dev, int32_t width, int32_t stack_limit, const struct Node2* nodes,
                                              int32_t num_nodes, const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes,
                                              struct Tri4* packets, void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch; RODENT_BUILD_ERR_INPUT when the device raised a flag. */
int32_t rodent_hip_collapse_bvh2_tri1_bounded_sync(int32_t dev, int32_t width, int32_t stack_limit, const struct Node2* nodes,
                                                   int32_t num_nodes, const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes,
                                                   struct Tri4* packets, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* RODENT_BUILD_H */
