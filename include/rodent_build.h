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

#ifdef __cplusplus
}
#endif
#endif /* RODENT_BUILD_H */
