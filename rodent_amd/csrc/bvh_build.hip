// bvh_build.hip -- BVH builder on the device writing BVH2 / Tri1 in the layout of include/rodent_traversal.h: a linear BVH (Morton
// codes + Karras 2012 hierarchy), optionally restructured by treelets with an SAH leaf collapse, optionally over pre-split triangles.
// C ABI: include/rodent_build.h.  CPU models of every stage, byte for byte: tests/lbvh_model.py, tests/trbvh_model.py (treelets),
// tests/split_model.py (pre-splitting), tests/refit_model.py and tests/refit_wide_model.py (refit).
// The kernels lie in build_device.h (what the stages share), build_lbvh.h, build_treelet.h, build_split.h, build_ploc.h, build_refit.h
// and build_collapse.h; build_tlas.h holds the instance and leaf stages of an instanced scene's top level (rodent_hip_build_tlas,
// include/rodent_instances.h; CPU model: tests/instance_model.py), which runs the LBVH's sort, Karras and tail stages over instance boxes.
// One pipeline (launch_build), all on the caller's stream, nothing allocated, no host synchronisation.  The four entry points only
// choose its options: rodent_hip_build_bvh2_tri1 the LBVH, _opt treelet_passes (0, or one triangle: the LBVH), _split the split front,
// _ploc the topology stage.
// Front, one of:
//   k_centroids      per triangle: indices checked before any vertex load, centroid sum s = (v0 + v1) + v2, per-block min / max
//   k_bounds         one block: the centroid bounds and per-axis scale = 1024 / extent (0 for an empty or non-finite extent)
// or (split) the pre-splitting stages of build_split.h, k_split_boxes ... k_refs, which make the n' references, then k_bounds over
// their Morton points.
// Tree (launch_tree):
//   k_morton         30-bit Morton code: cell = (uint)min(max((s - lo) * scale, 0), 1023) per axis, x in the highest bit of a triple
//   k_radix_*        stable LSD radix sort of (code, triangle id), 4 passes of 8 bits: order = by code, then by triangle id
//   k_leaves         Tri1 records in sorted order + the sorted triangles' boxes
//   k_karras         the n - 1 internal nodes (Karras 2012, delta ties broken by the sorted position), parent links, kept-node counts
// Tail, the LBVH's (treelet_passes = 0, launch_lbvh_tail):
//   k_renumber       kept internal nodes (more than max_leaf triangles) numbered by an exclusive scan in Karras order
//   k_bottom_up      boxes and heights, per-node arrival counters (first arriver leaves, the second goes on; no waiting)
//   k_emit / k_emit_root   Node2 records, end-of-leaf bits
// or the optimising one (treelet_passes > 0, launch_opt_tail):
//   k_explicit       the Karras tree as an explicit binary tree: left / right child ids (leaves: m + sorted position), parents
//   k_fit            bottom-up: box, triangle count, height, SAH cost, emitted-node count per inner node (arrival counters)
//   per pass k:      k_depth (every node's depth, a walk up the parent links), then k_treelet with gamma = 7 << k: the bottom-up
//                    climb again; each node of at least gamma triangles gets its 7-leaf treelet restructured by its wave
//   k_fit            again: the SAH leaf collapse decisions and emitted-node counts of the final tree
//   k_emit_opt_nodes / k_emit_opt_tris   Node2 in depth-first pre-order, Tri1 in left-to-right leaf order (O(depth) walks)
// PLOC (build_ploc.h, rodent_hip_build_bvh2_tri1_ploc; CPU model: tests/ploc_model.py): in place of k_karras and k_explicit, the explicit
// tree comes from locally-ordered clustering of the sorted references (k_ploc_init, per device-wide iteration k_ploc_nn, k_ploc_flags,
// k_scan, k_ploc_compact, then k_ploc_shrink and k_ploc_finish, one workgroup each); the optimising tail follows as it stands.
// Split, n' is known on the device only: the tree and tail stages get grids sized for max_refs and read n' (`nref`) from info[4];
// without `nref` the host sizes them for the n triangles.
// Refit (build_refit.h, rodent_hip_refit_bvh2_tri1): k_refit_links, k_refit_tris, k_refit_climb rewrite the boxes and Tri1 records of an
// existing hierarchy in place from moved vertices; the topology stays.  rodent_hip_refit_bvh4_tri4 / _bvh8_tri4 do the same for
// Node4 / Node8 + Tri4 (k_refit_wide_links, k_refit_tri4, k_refit_wide_climb; CPU model: tests/refit_wide_model.py).
// rodent_hip_refit_objects (include/rodent_instances.h) refits a listed subset of the packed objects of an instanced scene in the same
// three launches, whatever their number (k_forest_links, k_forest_tris, k_forest_climb).
// rodent_hip_build_motion_bvh2_tri1 (include/rodent_motion.h; build_motion.h; CPU model: tests/motion_bvh_model.py): two copies of a
// topology refitted to a mesh's two keys, then k_fuse_motion writes the two-key records a time per ray is traced through.
// rodent_hip_build_motion_objects (include/rodent_instances.h, "deforming objects under moving instances"; CPU model:
// tests/motion_objects_model.py) is its forest form: the packed arrays copied twice, rodent_hip_refit_objects' launches at either key,
// k_fuse_motion over the packed arrays; rodent_hip_build_motion_tlas_motion_objects is the motion TLAS over such a set.
// rodent_hip_build_objects (build_forest.h; CPU model: tests/forest_build_model.py) BUILDS a listed subset of the packed objects, or all
// objects of a new set, in one launch list whatever their number: the LBVH's stages over the objects' triangles laid end to end
// (k_bf_*), each object in its own frame, sorted by (list rank, code, row), every Karras position object-local.
// Collapse (build_collapse.h, rodent_hip_collapse_bvh2_tri1): any BVH2 / Tri1 becomes Node4 / Node8 + Tri4 by bounded walks per node,
// no thread waiting for another (CPU model: tests/collapse_model.py); rodent_hip_collapse_bvh2_tri1_bounded: the same under a stack limit
// (tests/collapse_bounded_model.py).
// Every value is a function of the inputs alone: min / max are exact and do not depend on the order they are taken in, the sort is
// stable, and arrival order decides only WHICH thread computes a node, never what it computes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rodent_build.h"
#include "rodent_instances.h"
#include "rodent_motion.h"

namespace {
#include "build_device.h"

// ---- scratch layouts: one carving each, shared by the *_scratch_bytes entry and the launcher ----------------------------------------
// Arrays one behind the other from `base`, each starting on a 256-byte boundary; without a base only the bytes are counted.
struct Carver {
    char* base; size_t bytes = 0;
    template <class T> void take(T*& array, size_t count) {
        array = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += (sizeof(T) * count + 255) & ~size_t(255);
    }
};

struct Scratch {
    uint32_t *keys[2], *vals[2];
    uint32_t* hist;               // 256 x radix tiles (digit-major), scanned in place
    float* partial;               // kBoundsBlocks x 6
    float* frame;                 // lo[3], scale[3]
    float4* cent;                 // per triangle: centroid sum (w unused)
    float* leafbox;               // per sorted position: lo_x hi_x lo_y hi_y lo_z hi_z
    int *first, *last, *split, *parent, *leaf_parent, *height, *newidx;
    float* box;                   // per internal node, same layout as leafbox
    uint32_t* arrivals;           // per internal node (zeroed for every call)
    uint32_t* blockcount;         // kept nodes per block of k_karras, scanned in place
    // the optimising builder only (carved behind the arrays above, so the LBVH's scratch size does not change)
    int *left, *right, *count, *emitted, *depth;
    float* cost;
    size_t bytes;
};

inline int radix_tiles(int n) { return (n + kRadixTile - 1) / kRadixTile; }

Scratch carve(char* base, int n, bool opt = false) {
    Scratch s{};
    Carver c{base};
    const size_t N = (size_t)n, M = (size_t)std::max(n - 1, 1);
    for (int k = 0; k < 2; k++) { c.take(s.keys[k], N); c.take(s.vals[k], N); }
    c.take(s.hist, 256 * (size_t)radix_tiles(n)); c.take(s.partial, 6 * kBoundsBlocks); c.take(s.frame, 8);
    c.take(s.cent, N); c.take(s.leafbox, 6 * N);
    c.take(s.first, M); c.take(s.last, M); c.take(s.split, M); c.take(s.parent, M);
    c.take(s.leaf_parent, N); c.take(s.height, M); c.take(s.newidx, M);
    c.take(s.box, 6 * M); c.take(s.arrivals, M); c.take(s.blockcount, (M + kBlock - 1) / kBlock);
    if (opt) { c.take(s.left, M); c.take(s.right, M); c.take(s.count, M); c.take(s.emitted, M); c.take(s.depth, M); c.take(s.cost, M); }
    s.bytes = c.bytes;
    return s;
}

struct SplitScratch {
    float* tbox;                  // per triangle: its box (canonical zeros)
    float* prio;                  // per triangle: p
    uint32_t *w, *s, *start, *made;
    uint32_t *blocktot, *blockmade;   // per block of kBlock triangles: sum of s + 1 / of the pieces made, scanned in place
    float* kpartial;              // per block: bounds of the references' Morton points
    float* sframe;                // lo[3], step[3]
    uint32_t* pmax;               // the bits of max p (p >= 0: integer order is float order); followed by W (uint64)
    unsigned long long* wsum;
    float* pbox;                  // per slot: a piece's box (the front of a triangle's range) or a pending piece (the back)
    int* pk;                      // per slot: a pending piece's splits
    float* refbox;                // per reference: its box
    int* reftri;                  // per reference: its triangle
    size_t bytes;
};

SplitScratch carve_split(char* base, int n, int max_refs) {
    SplitScratch q{};
    Carver c{base};
    const size_t N = (size_t)n, R = (size_t)max_refs, NB = (N + kBlock - 1) / kBlock;
    c.take(q.tbox, 6 * N); c.take(q.prio, N); c.take(q.w, N); c.take(q.s, N); c.take(q.start, N); c.take(q.made, N);
    c.take(q.blocktot, NB); c.take(q.blockmade, NB); c.take(q.kpartial, 6 * NB); c.take(q.sframe, 8);
    c.take(q.pmax, 4); q.wsum = q.pmax ? (unsigned long long*)(q.pmax + 2) : nullptr;
    c.take(q.pbox, 6 * R); c.take(q.pk, R); c.take(q.refbox, 6 * R); c.take(q.reftri, R);
    q.bytes = c.bytes;
    return q;
}

struct RefitScratch {
    int* parent;                  // per node: 2 * parent + slot, -1 = none (the root)
    uint32_t* arrivals;           // per node
    float* tribox;                // per Tri1 record: the box of its triangle; per Tri4 packet: the box of its valid lanes
    size_t bytes;
};

RefitScratch carve_refit(char* base, int num_nodes, int num_bvh_tris) {
    RefitScratch s{};
    Carver c{base};
    c.take(s.parent, (size_t)num_nodes); c.take(s.arrivals, (size_t)num_nodes); c.take(s.tribox, 6 * (size_t)num_bvh_tris);
    s.bytes = c.bytes;
    return s;
}

// rodent_hip_build_motion_bvh2_tri1: the two copies of the topology, the two refits' info words (A's four, then B's), and ONE refit
// scratch, which the two refits use one after the other on the call's stream.
struct MotionScratch {
    Node2* nodes[2];
    Tri1* tris[2];
    int32_t* refit_info;
    char* refit;
    size_t bytes;
};

// (rodent_hip_build_motion_objects carves the same way over the packed arrays, with the refit scratch of its plan: `refit_bytes`)
MotionScratch carve_motion(char* base, int num_nodes, int num_bvh_tris, size_t refit_bytes) {
    MotionScratch s{};
    Carver c{base};
    for (int k = 0; k < 2; k++) { c.take(s.nodes[k], (size_t)num_nodes); c.take(s.tris[k], (size_t)num_bvh_tris); }
    c.take(s.refit_info, 2 * RODENT_BUILD_INFO_WORDS);
    c.take(s.refit, refit_bytes);
    s.bytes = c.bytes;
    return s;
}

MotionScratch carve_motion(char* base, int num_nodes, int num_bvh_tris) {
    return carve_motion(base, num_nodes, num_bvh_tris, carve_refit(nullptr, num_nodes, num_bvh_tris).bytes);
}

struct CollapseScratch {
    int* parent;                  // per node, as RefitScratch
    uint32_t* arrivals;           // per node: k_refit_links zeroes it, nobody arrives
    int *small, *small_first, *root;
    uint32_t *wide_id, *nodetot;  // per node / per block of nodes
    int* mark;                    // per Tri1 record
    uint32_t *packet_id, *rectot; // per record / per block of records
    int *height, *above;          // per node, behind everything else: only a collapse with a stack limit has them
    size_t bytes;
};

CollapseScratch carve_collapse(char* base, int num_nodes, int num_bvh_tris, bool bounded) {
    CollapseScratch s{};
    Carver c{base};
    const size_t N = (size_t)num_nodes, T = (size_t)num_bvh_tris;
    c.take(s.parent, N); c.take(s.arrivals, N); c.take(s.small, N); c.take(s.small_first, N); c.take(s.root, N);
    c.take(s.wide_id, N); c.take(s.nodetot, (N + kBlock - 1) / kBlock);
    c.take(s.mark, T); c.take(s.packet_id, T); c.take(s.rectot, (T + kBlock - 1) / kBlock);
    if (bounded) { c.take(s.height, N); c.take(s.above, N); }
    s.bytes = c.bytes;
    return s;
}

template <class Rec>               // RodentInstance or RodentMotionInstance
struct TlasScratch {
    Rec* staged;                  // per descriptor: its record, before the sort
    float* wbox;                  // per descriptor: its world box (its motion box)
    size_t bytes;
};

template <class Rec>
TlasScratch<Rec> carve_tlas(char* base, int n) {
    TlasScratch<Rec> t{};
    Carver c{base};
    c.take(t.staged, (size_t)n); c.take(t.wbox, 6 * (size_t)n);
    t.bytes = c.bytes;
    return t;
}

struct ForestBuildScratch {
    uint32_t *keys[2], *vals[2];
    uint32_t* hist;               // 256 x radix tiles (digit-major), scanned in place
    uint32_t *code0, *codes;      // per unsorted / per sorted position: its Morton code
    float4* cent;                 // per unsorted position: centroid sum (w unused)
    float* leafbox;               // per sorted position
    int *first, *last, *split, *parent, *leaf_parent, *height;    // per position: the object's Karras node of that local index
    uint32_t* gidx;               // per position: kept nodes in front of it, over all objects
    float* box;                   // per position, as leafbox
    uint32_t* arrivals;           // per position (zeroed for every call)
    uint32_t* blockcount;         // kept nodes per block of k_bf_karras, scanned in place
    uint32_t* fbounds;            // 6 per listed object
    uint32_t* objnodes;           // per listed object
    size_t bytes;
};

ForestBuildScratch carve_forest_build(char* base, int total_tris, int num_listed) {
    ForestBuildScratch s{};
    Carver c{base};
    const size_t N = (size_t)total_tris, K = (size_t)num_listed;
    for (int k = 0; k < 2; k++) { c.take(s.keys[k], N); c.take(s.vals[k], N); }
    c.take(s.hist, 256 * (size_t)radix_tiles(total_tris)); c.take(s.code0, N); c.take(s.codes, N); c.take(s.cent, N);
    c.take(s.leafbox, 6 * N);
    c.take(s.first, N); c.take(s.last, N); c.take(s.split, N); c.take(s.parent, N); c.take(s.leaf_parent, N); c.take(s.height, N);
    c.take(s.gidx, N); c.take(s.box, 6 * N); c.take(s.arrivals, N); c.take(s.blockcount, (N + kBlock - 1) / kBlock);
    c.take(s.fbounds, 6 * K); c.take(s.objnodes, K);
    s.bytes = c.bytes;
    return s;
}

struct PlocScratch {
    float4* clusters[2];          // per position, the two cluster buffers: a 32-byte record (build_ploc.h: PlocCluster)
    int* nn;                      // per position
    uint32_t* blocktot;           // leader and survivor counts per block of positions
    int* state;                   // C and t, two slots; the finisher's hand-over
    size_t bytes;
};

PlocScratch carve_ploc(char* base, int max_refs) {
    PlocScratch s{};
    Carver c{base};
    const size_t R = (size_t)max_refs;
    for (int k = 0; k < 2; k++) c.take(s.clusters[k], 2 * R);
    c.take(s.nn, R); c.take(s.blocktot, 2 * ((R + kBlock - 1) / kBlock)); c.take(s.state, 8);
    s.bytes = c.bytes;
    return s;
}

#include "build_lbvh.h"
#include "instance_inverse.h"
#include "build_tlas.h"
#include "build_treelet.h"
#include "build_split.h"
#include "build_ploc.h"
#include "build_refit.h"
#include "build_motion.h"
#include "build_forest.h"
#include "build_collapse.h"

inline int blocks_for(long long items) { return (int)((items + kBlock - 1) / kBlock); }

bool set_device(int32_t dev) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && dev >= 0 && dev < count && hipSetDevice(dev) == hipSuccess;
}

bool bad_num_tris(int32_t num_tris) { return num_tris < 1 || num_tris > kMaxTris; }

int32_t check_args(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris, int32_t max_leaf,
                   const void* nodes, const void* tris, const void* scratch, const int32_t* info_dev) {
    if (bad_num_tris(num_tris)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (max_leaf < 1 || max_leaf > 8) return RODENT_BUILD_ERR_MAX_LEAF;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (!vertices || !indices || !nodes || !tris || !scratch || !info_dev) return RODENT_BUILD_ERR_NULL;
    return set_device(dev) ? RODENT_BUILD_OK : RODENT_BUILD_ERR_DEVICE;
}

int32_t check_options(const RodentBuildOptions* opt) {
    if (!opt) return RODENT_BUILD_ERR_NULL;
    if (opt->max_leaf < 1 || opt->max_leaf > RODENT_BUILD_MAX_LEAF) return RODENT_BUILD_ERR_MAX_LEAF;
    if (opt->treelet_passes < 0 || opt->treelet_passes > RODENT_BUILD_MAX_TREELET_PASSES) return RODENT_BUILD_ERR_PASSES;
    if (!(opt->node_cost > 0.0f && opt->node_cost <= 1e6f) || !(opt->tri_cost > 0.0f && opt->tri_cost <= 1e6f))
        return RODENT_BUILD_ERR_COST;
    return RODENT_BUILD_OK;
}

int32_t check_split(const RodentSplitOptions* split) {
    if (!split) return RODENT_BUILD_ERR_NULL;
    if (!(split->budget >= 0.0f && split->budget <= RODENT_BUILD_MAX_SPLIT_BUDGET)) return RODENT_BUILD_ERR_SPLIT;   // NaN too
    if (split->max_pieces < 1 || split->max_pieces > RODENT_BUILD_MAX_PIECES) return RODENT_BUILD_ERR_SPLIT;
    return RODENT_BUILD_OK;
}

// B = min(floor(budget * n), 2^25 - n): the product of a float and an int below 2^25 is exact in double
long long split_budget(int n, const RodentSplitOptions* split) {
    return std::min((long long)std::floor((double)split->budget * (double)n), (long long)kMaxTris - n);
}

long long split_max_refs(int n, const RodentSplitOptions* split) {
    return n + std::min(split_budget(n, split), (long long)n * (split->max_pieces - 1));
}

int host_clog2(long long x) { int k = 0; while ((1LL << k) < x) k++; return k; }

// The PLOC options' own checks; with num_tris in range also D >= clog2(the most references).
int32_t check_ploc(const RodentPlocOptions* ploc, const RodentBuildOptions* opt, const RodentSplitOptions* split, int32_t num_tris) {
    if (!ploc) return RODENT_BUILD_ERR_NULL;
    if (ploc->radius < 1 || ploc->radius > RODENT_BUILD_MAX_PLOC_RADIUS || ploc->depth_limit < 0
        || ploc->depth_limit > RODENT_BUILD_MAX_DEPTH || ploc->wide_iterations < -1 || ploc->wide_iterations > 255)
        return RODENT_BUILD_ERR_PLOC;
    const int D = ploc->depth_limit ? ploc->depth_limit : RODENT_BUILD_MAX_DEPTH;
    if (D < RODENT_BUILD_MAX_DEPTH && opt->treelet_passes > 0) return RODENT_BUILD_ERR_PLOC;
    if (!bad_num_tris(num_tris) && D < host_clog2(split ? split_max_refs(num_tris, split) : num_tris)) return RODENT_BUILD_ERR_PLOC;
    return RODENT_BUILD_OK;
}

// The device-wide iterations before the finisher: about 0.75 of the clusters are left after one, so 4 per halving beyond the 1024
// clusters the finisher keeps in LDS.
int ploc_wide_iterations(const RodentPlocOptions& ploc, int max_refs) {
    if (ploc.wide_iterations >= 0) return ploc.wide_iterations;
    return std::min(255, 4 * std::max(0, host_clog2(max_refs) - 10));
}

// The optimising stages' view of the scratch arrays for n references.
Opt make_opt(const Scratch& s, int n, const RodentBuildOptions& opt, const int* nref) {
    Opt o{};
    o.n = n; o.m = n - 1; o.max_leaf = opt.max_leaf; o.node_cost = opt.node_cost; o.tri_cost = opt.tri_cost; o.nref = nref;
    o.left = s.left; o.right = s.right; o.parent = s.parent; o.leaf_parent = s.leaf_parent; o.count = s.count; o.height = s.height;
    o.emitted = s.emitted; o.depth = s.depth; o.box = s.box; o.cost = s.cost; o.leafbox = s.leafbox;
    return o;
}

// launch_tree: Morton codes (from s.cent and s.frame) and the sort (launch_sort), the sorted leaves and (n > 1) the Karras hierarchy
// (launch_karras); the TLAS build (launch_tlas) puts its own leaf stage between the two.  With `nref` (split) the grids are sized for
// n = max_refs and every kernel runs over the n' = *nref references (reftri / refbox: their triangles and boxes).
void launch_sort(const Scratch& s, int n, const int* nref, hipStream_t stream) {
    hipLaunchKernelGGL(k_morton, dim3(blocks_for(n)), dim3(kBlock), 0, stream, s.cent, n, s.frame, s.keys[0], s.vals[0], nref);
    const int tiles = radix_tiles(n);
    for (int pass = 0; pass < 4; pass++) {                       // 30 key bits: 8 + 8 + 8 + 6; four passes end in buffer 0
        const int in = pass & 1, shift = 8 * pass;
        hipLaunchKernelGGL(k_radix_hist, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], n, shift, s.hist, nref);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.hist, 256 * tiles, (int*)nullptr);
        hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], s.vals[in], s.keys[in ^ 1],
                           s.vals[in ^ 1], s.hist, n, shift, nref);
    }
}

void launch_karras(const Scratch& s, int n, int max_leaf, const int* nref, hipStream_t stream) {
    const int m = n - 1;
    if (m > 0)
        hipLaunchKernelGGL(k_karras, dim3(blocks_for(m)), dim3(kBlock), 0, stream, s.keys[0], n, max_leaf, s.first, s.last, s.split,
                           s.parent, s.leaf_parent, s.blockcount, nref);
}

void launch_tree(const Scratch& s, const float4* v4, int nv, const int4* i4, int n, int max_leaf, Tri1* tris, const int* nref,
                 const int* reftri, const float* refbox, bool karras, hipStream_t stream) {
    launch_sort(s, n, nref, stream);
    hipLaunchKernelGGL(k_leaves, dim3(blocks_for(n)), dim3(kBlock), 0, stream, v4, nv, i4, s.vals[0], n, tris, s.leafbox, nref,
                       reftri, refbox);
    if (karras) launch_karras(s, n, max_leaf, nref, stream);
}

// The PLOC topology stage over n (or, with `nref`, at most n) sorted references: the clusters of iteration 0, `wide` device-wide
// iterations, the two finishing kernels.  The list depends on n and `wide` alone.
void launch_ploc(const Scratch& s, const PlocScratch& c, int n, const RodentPlocOptions& ploc, int wide, int32_t* info_dev, const int* nref,
                 hipStream_t stream) {
    Ploc p{};
    p.n = n; p.m = n - 1; p.radius = ploc.radius; p.depth_limit = ploc.depth_limit; p.nblocks = blocks_for(n); p.nref = nref;
    p.leafbox = s.leafbox; p.left = s.left; p.right = s.right; p.parent = s.parent; p.leaf_parent = s.leaf_parent;
    p.buf0 = reinterpret_cast<PlocCluster*>(c.clusters[0]); p.buf1 = reinterpret_cast<PlocCluster*>(c.clusters[1]);
    p.nn = c.nn; p.blocktot = c.blocktot; p.state = c.state; p.info = info_dev;
    hipLaunchKernelGGL(k_ploc_init, dim3(p.nblocks), dim3(kBlock), 0, stream, p);
    if (n < 2) return;
    for (int k = 0; k < wide; k++) {
        hipLaunchKernelGGL(k_ploc_nn, dim3(p.nblocks), dim3(kBlock), 0, stream, p, k);
        hipLaunchKernelGGL(k_ploc_flags, dim3(p.nblocks), dim3(kBlock), 0, stream, p, k);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, c.blocktot, 2 * p.nblocks, (int*)nullptr);
        hipLaunchKernelGGL(k_ploc_compact, dim3(p.nblocks), dim3(kBlock), 0, stream, p, k);
    }
    hipLaunchKernelGGL(k_ploc_shrink, dim3(1), dim3(kPlocFinish), 0, stream, p, wide);
    hipLaunchKernelGGL(k_ploc_finish, dim3(1), dim3(kPlocFinish), 0, stream, p);
}

// The LBVH tail: renumbering, boxes and heights, Node2 records.  Without `nref` the host knows n and launches either k_emit or the
// single-leaf root; with it both are launched and each writes only when n' calls for it.
template <class Rec>
void launch_lbvh_tail(const Scratch& s, int n, int max_leaf, Node2* nodes, Rec* tris, int32_t* info_dev, const int* nref,
                      hipStream_t stream) {
    const int m = n - 1;
    if (m > 0) {
        const int kblocks = blocks_for(m);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.blockcount, kblocks, info_dev + kInfoNodes);
        hipLaunchKernelGGL(k_renumber, dim3(kblocks), dim3(kBlock), 0, stream, s.first, s.last, m, max_leaf, s.blockcount, s.newidx,
                           nref);
        hipLaunchKernelGGL(k_bottom_up, dim3(blocks_for(n)), dim3(kBlock), 0, stream, n, max_leaf, s.first, s.last, s.split, s.parent,
                           s.leaf_parent, s.leafbox, s.box, s.height, s.arrivals, info_dev, nref);
    }
    if (nref ? m > 0 : n > max_leaf)
        hipLaunchKernelGGL(k_emit<Rec>, dim3(blocks_for(m)), dim3(kBlock), 0, stream, m, s.first, s.last, s.split, s.newidx, s.leafbox,
                           s.box, nodes, tris, nref);
    if (nref || n <= max_leaf)
        hipLaunchKernelGGL(k_emit_root<Rec>, dim3(1), dim3(1), 0, stream, n, s.leafbox, s.box, nodes, tris, info_dev, nref, max_leaf);
}

// The optimising tail: the explicit tree, k_fit, the treelet passes, k_fit again, pre-order emission.  Without `nref` it is only
// reached with n > 1; with it the single-leaf root follows, written when n' = 1.  False when a memset is refused.
bool launch_opt_tail(const Scratch& s, int n, const RodentBuildOptions& opt, const float4* v4, int nv, const int4* i4, Node2* nodes,
                     Tri1* tris, int32_t* info_dev, const int* nref, const int* reftri, bool karras, hipStream_t stream) {
    const int m = n - 1;
    if (m > 0) {
        const Opt o = make_opt(s, n, opt, nref);
        if (karras)                                              // PLOC has written the explicit tree itself
            hipLaunchKernelGGL(k_explicit, dim3(blocks_for(m)), dim3(kBlock), 0, stream, m, s.first, s.last, s.split, s.left, s.right,
                               nref);
        hipLaunchKernelGGL(k_fit, dim3(blocks_for(n)), dim3(kBlock), 0, stream, o, s.arrivals);
        for (int pass = 0; pass < opt.treelet_passes; pass++) {
            hipLaunchKernelGGL(k_depth, dim3(blocks_for(m)), dim3(kBlock), 0, stream, o);
            if (hipMemsetAsync(s.arrivals, 0, 4 * (size_t)m, stream) != hipSuccess) return false;
            hipLaunchKernelGGL(k_treelet, dim3((n + 63) / 64), dim3(64), 0, stream, o, kTreelet << pass, s.arrivals, info_dev);
        }
        if (hipMemsetAsync(s.arrivals, 0, 4 * (size_t)m, stream) != hipSuccess) return false;
        hipLaunchKernelGGL(k_fit, dim3(blocks_for(n)), dim3(kBlock), 0, stream, o, s.arrivals);
        hipLaunchKernelGGL(k_emit_opt_nodes, dim3(blocks_for(m)), dim3(kBlock), 0, stream, o, nodes, info_dev);
        hipLaunchKernelGGL(k_emit_opt_tris, dim3(blocks_for(n)), dim3(kBlock), 0, stream, o, v4, nv, i4, s.vals[0], tris, reftri);
    }
    // one reference (one triangle, not cut): the single-leaf form, as the LBVH writes it for one triangle
    if (nref) hipLaunchKernelGGL(k_emit_root<Tri1>, dim3(1), dim3(1), 0, stream, n, s.leafbox, s.box, nodes, tris, info_dev, nref, 1);
    return true;
}

// Every entry after its argument checks: info words and arrival counters zeroed, the front (centroids, or with `split` the
// pre-splitting stages of build_split.h), launch_tree, then the LBVH tail (treelet_passes = 0) or the optimising one.  Without `split`
// the stages run over the n triangles; with it over the n' references, on grids sized for max_refs.  With `ploc` the topology stage is
// PLOC instead of Karras' and the tail the optimising one whatever treelet_passes; one reference at most: the LBVH's single leaf.
int32_t launch_build(const float* vertices, int nv, const int32_t* indices, int n, const RodentBuildOptions& opt,
                     const RodentSplitOptions* split, const RodentPlocOptions* ploc, Node2* nodes, Tri1* tris, void* scratch,
                     int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int R = split ? (int)split_max_refs(n, split) : n, M = R - 1;
    const bool optimise = ploc ? R > 1 : opt.treelet_passes > 0;
    const Scratch s = carve(static_cast<char*>(scratch), R, optimise || ploc);
    const SplitScratch q = split ? carve_split(static_cast<char*>(scratch) + s.bytes, n, R) : SplitScratch{};
    const PlocScratch c = ploc ? carve_ploc(static_cast<char*>(scratch) + s.bytes + q.bytes, R) : PlocScratch{};
    const float4* v4 = reinterpret_cast<const float4*>(vertices);
    const int4* i4 = reinterpret_cast<const int4*>(indices);
    const int* nref = split ? info_dev + kInfoRefs : nullptr;     // n', written by the second scan; every later stage reads it
    // an unsplit caller's info buffer may hold only RODENT_BUILD_INFO_WORDS words
    const size_t info_bytes = 4 * (size_t)(split || ploc ? RODENT_BUILD_SPLIT_INFO_WORDS : RODENT_BUILD_INFO_WORDS);
    if (hipMemsetAsync(info_dev, 0, info_bytes, stream) != hipSuccess
        || (M > 0 && hipMemsetAsync(s.arrivals, 0, 4 * (size_t)M, stream) != hipSuccess)
        || (split && hipMemsetAsync(q.pmax, 0, 16, stream) != hipSuccess))
        return RODENT_BUILD_ERR_LAUNCH;
    const int nb = blocks_for(n), cblocks = std::min(kBoundsBlocks, nb);
    if (!split) {
        hipLaunchKernelGGL(k_centroids, dim3(cblocks), dim3(kBlock), 0, stream, v4, nv, i4, n, s.cent, s.partial, info_dev);
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(kBlock), 0, stream, s.partial, cblocks, s.frame);
    } else {
        hipLaunchKernelGGL(k_split_boxes, dim3(cblocks), dim3(kBlock), 0, stream, v4, nv, i4, n, q.tbox, s.partial, info_dev);
        hipLaunchKernelGGL(k_split_frame, dim3(1), dim3(kBlock), 0, stream, s.partial, cblocks, q.sframe);
        hipLaunchKernelGGL(k_priority, dim3(nb), dim3(kBlock), 0, stream, v4, nv, i4, n, q.tbox, q.sframe, q.prio, q.pmax);
        hipLaunchKernelGGL(k_weights, dim3(nb), dim3(kBlock), 0, stream, q.prio, n, q.pmax, q.w, q.wsum);
        hipLaunchKernelGGL(k_allot, dim3(nb), dim3(kBlock), 0, stream, q.w, n, split_budget(n, split), split->max_pieces, q.wsum, q.s,
                           q.blocktot, info_dev);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, q.blocktot, nb, (int*)nullptr);
        hipLaunchKernelGGL(k_split, dim3(nb), dim3(kBlock), 0, stream, v4, nv, i4, n, q.tbox, q.sframe, q.s, q.blocktot, q.pbox, q.pk,
                           q.start, q.made, q.blockmade, info_dev);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, q.blockmade, nb, info_dev + kInfoRefs);
        hipLaunchKernelGGL(k_refs, dim3(nb), dim3(kBlock), 0, stream, v4, nv, i4, n, q.tbox, q.s, q.start, q.made, q.blockmade, q.pbox,
                           q.refbox, q.reftri, s.cent, q.kpartial);
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(kBlock), 0, stream, q.kpartial, nb, s.frame);
    }
    launch_tree(s, v4, nv, i4, R, opt.max_leaf, tris, nref, q.reftri, q.refbox, !ploc, stream);
    if (ploc) launch_ploc(s, c, R, *ploc, ploc_wide_iterations(*ploc, R), info_dev, nref, stream);
    if (!optimise)
        launch_lbvh_tail(s, R, opt.max_leaf, nodes, tris, info_dev, nref, stream);
    else if (!launch_opt_tail(s, R, opt, v4, nv, i4, nodes, tris, info_dev, nref, q.reftri, !ploc, stream))
        return RODENT_BUILD_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The TLAS build after its argument checks: info words and arrival counters zeroed, the instance stage and the frame of its sort points,
// the sort, the leaf stage, Karras and the LBVH tail over RodentInstance records -- or, with motion descriptors, the motion instance
// stage and RodentMotionInstance records.
inline auto instance_stage(const RodentInstanceDesc*, const Node2*) { return k_instances; }
inline auto instance_stage(const RodentMotionInstanceDesc*, const Node2*) { return k_motion_instances<Node2>; }
inline auto instance_stage(const RodentMotionInstanceDesc*, const RodentMotionNode2*) { return k_motion_instances<RodentMotionNode2>; }

template <class ObjNode, class Desc, class Rec>
int32_t launch_tlas(const ObjNode* nodes, const RodentObject* objects, int num_objects, const Desc* descs, int n, int max_leaf,
                    Node2* tlas_nodes, Rec* instances, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Scratch s = carve(static_cast<char*>(scratch), n);
    const TlasScratch<Rec> t = carve_tlas<Rec>(static_cast<char*>(scratch) + s.bytes, n);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || (n > 1 && hipMemsetAsync(s.arrivals, 0, 4 * (size_t)(n - 1), stream) != hipSuccess))
        return RODENT_BUILD_ERR_LAUNCH;
    const int cblocks = std::min(kBoundsBlocks, blocks_for(n));
    hipLaunchKernelGGL(instance_stage(descs, nodes), dim3(cblocks), dim3(kBlock), 0, stream, nodes, objects, num_objects, descs, n, t.staged,
                       t.wbox, s.cent, s.partial, info_dev);
    hipLaunchKernelGGL(k_bounds, dim3(1), dim3(kBlock), 0, stream, s.partial, cblocks, s.frame);
    launch_sort(s, n, nullptr, stream);
    hipLaunchKernelGGL(k_tlas_leaves<Rec>, dim3(blocks_for(n)), dim3(kBlock), 0, stream, t.staged, t.wbox, s.vals[0], n, instances, s.leafbox);
    launch_karras(s, n, max_leaf, nullptr, stream);
    launch_lbvh_tail(s, n, max_leaf, tlas_nodes, instances, info_dev, nullptr, stream);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The refit after its argument checks: info words zeroed, parent slots set to -1, then the three kernels of build_refit.h.
int32_t launch_refit(const float* vertices, int nv, const int32_t* indices, int n, Node2* nodes, int num_nodes, Tri1* tris,
                     int num_bvh_tris, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const RefitScratch s = carve_refit(static_cast<char*>(scratch), num_nodes, num_bvh_tris);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || hipMemsetAsync(s.parent, 0xFF, 4 * (size_t)num_nodes, stream) != hipSuccess)
        return RODENT_BUILD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_refit_links, dim3(blocks_for(num_nodes)), dim3(kBlock), 0, stream, nodes, num_nodes, num_bvh_tris, s.parent,
                       s.arrivals, info_dev);
    hipLaunchKernelGGL(k_refit_tris, dim3(blocks_for(num_bvh_tris)), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(vertices),
                       nv, reinterpret_cast<const int4*>(indices), n, tris, num_bvh_tris, s.tribox, info_dev);
    hipLaunchKernelGGL(k_refit_climb, dim3(blocks_for(num_nodes)), dim3(kBlock), 0, stream, nodes, num_nodes, tris, num_bvh_tris,
                       s.tribox, s.parent, s.arrivals, info_dev);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The fuse after its argument checks: info words zeroed (unless the build did), one launch.
int32_t launch_fuse_motion(const Node2* nodes0, const Tri1* tris0, const Node2* nodes1, const Tri1* tris1, int num_nodes, int num_bvh_tris,
                           RodentMotionNode2* motion_nodes, RodentMotionTri1* motion_tris, const int32_t* refit_info, int32_t* info_dev,
                           void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_fuse_motion, dim3(blocks_for((long long)num_nodes + num_bvh_tris)), dim3(kBlock), 0, stream, nodes0, tris0, nodes1,
                       tris1, num_nodes, num_bvh_tris, motion_nodes, motion_tris, refit_info, info_dev);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The motion build after its argument checks: the fixed list of include/rodent_motion.h.
int32_t launch_motion_build(const float* vertices0, const float* vertices1, int nv, const int32_t* indices, int n, const Node2* nodes,
                            int num_nodes, const Tri1* tris, int num_bvh_tris, RodentMotionNode2* motion_nodes,
                            RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const MotionScratch s = carve_motion(static_cast<char*>(scratch), num_nodes, num_bvh_tris);
    for (int k = 0; k < 2; k++) {
        // (the whole topology, copy B's too, before the first refit: what is refitted in place never feeds a copy)
        if (hipMemcpyAsync(s.nodes[k], nodes, sizeof(Node2) * (size_t)num_nodes, hipMemcpyDeviceToDevice, stream) != hipSuccess
            || hipMemcpyAsync(s.tris[k], tris, sizeof(Tri1) * (size_t)num_bvh_tris, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return RODENT_BUILD_ERR_LAUNCH;
    }
    const float* keys[2] = {vertices0, vertices1};
    for (int k = 0; k < 2; k++) {
        const int32_t rc = launch_refit(keys[k], nv, indices, n, s.nodes[k], num_nodes, s.tris[k], num_bvh_tris, s.refit,
                                        s.refit_info + k * RODENT_BUILD_INFO_WORDS, stream_);
        if (rc != RODENT_BUILD_OK) return rc;
    }
    return launch_fuse_motion(s.nodes[0], s.tris[0], s.nodes[1], s.tris[1], num_nodes, num_bvh_tris, motion_nodes, motion_tris,
                              s.refit_info, info_dev, stream_);
}

// The refit of the listed objects of a packed set after its argument checks: launch_refit's list over the listed objects' nodes and
// records laid end to end, whatever their number.  The links launch also covers one thread per range (the ranges' own flags).
int32_t launch_refit_objects(const float* vertices, int nv, const int32_t* indices, Node2* nodes, Tri1* tris, const ForestArgs& a,
                             void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const RefitScratch s = carve_refit(static_cast<char*>(scratch), a.total_nodes, a.total_recs);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || (a.total_nodes > 0 && hipMemsetAsync(s.parent, 0xFF, 4 * (size_t)a.total_nodes, stream) != hipSuccess))
        return RODENT_BUILD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_forest_links, dim3(blocks_for(std::max(a.total_nodes, a.num_listed))), dim3(kBlock), 0, stream, nodes, a,
                       s.parent, s.arrivals, info_dev);
    if (a.total_recs > 0)
        hipLaunchKernelGGL(k_forest_tris, dim3(blocks_for(a.total_recs)), dim3(kBlock), 0, stream,
                           reinterpret_cast<const float4*>(vertices), nv, reinterpret_cast<const int4*>(indices), tris, a, s.tribox,
                           info_dev);
    if (a.total_nodes > 0)
        hipLaunchKernelGGL(k_forest_climb, dim3(blocks_for(a.total_nodes)), dim3(kBlock), 0, stream, nodes, tris, a, s.tribox, s.parent,
                           s.arrivals, info_dev);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The motion build of a packed set after its argument checks: launch_motion_build's list with launch_refit_objects' in the place of
// launch_refit's, over the whole packed arrays (num_nodes / num_recs records); `a` lists every object.
int32_t launch_motion_objects(const float* vertices0, const float* vertices1, int nv, const int32_t* indices, const Node2* nodes,
                              int num_nodes, const Tri1* tris, int num_recs, const ForestArgs& a, RodentMotionNode2* motion_nodes,
                              RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const MotionScratch s = carve_motion(static_cast<char*>(scratch), num_nodes, num_recs, 0);      // (the refit scratch lies last)
    for (int k = 0; k < 2; k++) {
        if (hipMemcpyAsync(s.nodes[k], nodes, sizeof(Node2) * (size_t)num_nodes, hipMemcpyDeviceToDevice, stream) != hipSuccess
            || hipMemcpyAsync(s.tris[k], tris, sizeof(Tri1) * (size_t)num_recs, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return RODENT_BUILD_ERR_LAUNCH;
    }
    const float* keys[2] = {vertices0, vertices1};
    for (int k = 0; k < 2; k++) {
        const int32_t rc = launch_refit_objects(keys[k], nv, indices, s.nodes[k], s.tris[k], a, s.refit,
                                                s.refit_info + k * RODENT_BUILD_INFO_WORDS, stream_);
        if (rc != RODENT_BUILD_OK) return rc;
    }
    return launch_fuse_motion(s.nodes[0], s.tris[0], s.nodes[1], s.tris[1], num_nodes, num_recs, motion_nodes, motion_tris, s.refit_info,
                              info_dev, stream_);
}

// The build of the listed objects after its argument checks (build_forest.h): the info words and the arrival counters zeroed, then the
// LBVH's list over the listed objects' triangles laid end to end.  The list depends on the number of listed objects only through the
// rank passes of the sort: ceil(log2(num_listed) / 8) of them, none for one object.
int32_t launch_build_objects(const float* vertices, int nv, const int32_t* indices, Node2* nodes, Tri1* tris, BuildForest a, void* scratch,
                             void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int T = a.total_tris, K = a.num_listed, tb = blocks_for(T), kb = blocks_for(K), tiles = radix_tiles(T);
    const ForestBuildScratch s = carve_forest_build(static_cast<char*>(scratch), T, K);
    a.fbounds = s.fbounds; a.objnodes = s.objnodes;
    const float4* v4 = reinterpret_cast<const float4*>(vertices);
    const int4* i4 = reinterpret_cast<const int4*>(indices);
    if (hipMemsetAsync(a.info, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || hipMemsetAsync(s.arrivals, 0, 4 * (size_t)T, stream) != hipSuccess)
        return RODENT_BUILD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_bf_begin, dim3(kb), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(k_bf_centroids, dim3(tb), dim3(kBlock), 0, stream, v4, nv, i4, a, s.cent);
    hipLaunchKernelGGL(k_bf_morton, dim3(tb), dim3(kBlock), 0, stream, a, s.cent, s.code0, s.keys[0], s.vals[0]);
    int cur = 0;
    const auto radix_pass = [&](int shift) {
        hipLaunchKernelGGL(k_radix_hist, dim3(tiles), dim3(kBlock), 0, stream, s.keys[cur], T, shift, s.hist, (const int*)nullptr);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.hist, 256 * tiles, (int*)nullptr);
        hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kBlock), 0, stream, s.keys[cur], s.vals[cur], s.keys[cur ^ 1],
                           s.vals[cur ^ 1], s.hist, T, shift, (const int*)nullptr);
        cur ^= 1;
    };
    for (int pass = 0; pass < 4; pass++) radix_pass(8 * pass);           // by code: ties stay in (rank, row) order
    const int rank_passes = (host_clog2(K) + 7) / 8;
    if (rank_passes > 0) hipLaunchKernelGGL(k_bf_rank_keys, dim3(tb), dim3(kBlock), 0, stream, a, s.vals[cur], s.keys[cur]);
    for (int pass = 0; pass < rank_passes; pass++) radix_pass(8 * pass); // then, stably, by list rank
    hipLaunchKernelGGL(k_bf_leaves, dim3(tb), dim3(kBlock), 0, stream, v4, nv, i4, a, s.vals[cur], s.code0, tris, s.leafbox, s.codes);
    hipLaunchKernelGGL(k_bf_karras, dim3(tb), dim3(kBlock), 0, stream, a, s.codes, s.first, s.last, s.split, s.parent, s.leaf_parent,
                       s.blockcount);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.blockcount, tb, (int*)nullptr);
    hipLaunchKernelGGL(k_bf_renumber, dim3(tb), dim3(kBlock), 0, stream, a, s.first, s.last, s.blockcount, s.gidx);
    hipLaunchKernelGGL(k_bf_counts, dim3(kb), dim3(kBlock), 0, stream, a, s.gidx);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.objnodes, K, a.info + kInfoNodes);
    hipLaunchKernelGGL(k_bf_bottom_up, dim3(tb), dim3(kBlock), 0, stream, a, s.first, s.last, s.split, s.parent, s.leaf_parent,
                       s.leafbox, s.box, s.height, s.arrivals);
    hipLaunchKernelGGL(k_bf_emit, dim3(tb), dim3(kBlock), 0, stream, a, s.first, s.last, s.split, s.gidx, s.leafbox, s.box, nodes, tris);
    hipLaunchKernelGGL(k_bf_objects, dim3(kb), dim3(kBlock), 0, stream, a, s.leafbox, s.box, nodes, tris);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The same for Node4 / Node8 + Tri4: one launcher for both widths.
template <class Node>
int32_t launch_refit_wide(const float* vertices, int nv, const int32_t* indices, int n, Node* nodes, int num_nodes, Tri4* tris,
                          int num_packets, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const RefitScratch s = carve_refit(static_cast<char*>(scratch), num_nodes, num_packets);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || hipMemsetAsync(s.parent, 0xFF, 4 * (size_t)num_nodes, stream) != hipSuccess)
        return RODENT_BUILD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_refit_wide_links<Node>, dim3(blocks_for(num_nodes)), dim3(kBlock), 0, stream, nodes, num_nodes, num_packets,
                       s.parent, s.arrivals, info_dev);
    hipLaunchKernelGGL(k_refit_tri4, dim3(blocks_for(4LL * num_packets)), dim3(kBlock), 0, stream,
                       reinterpret_cast<const float4*>(vertices), nv, reinterpret_cast<const int4*>(indices), n, tris, num_packets,
                       s.tribox, info_dev);
    hipLaunchKernelGGL(k_refit_wide_climb<Node>, dim3(blocks_for(num_nodes)), dim3(kBlock), 0, stream, nodes, num_nodes, tris,
                       num_packets, s.tribox, s.parent, s.arrivals, info_dev);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// What the refit and collapse entries check of an existing hierarchy, in this order; `num_leaf_records`: Tri1 records or Tri4 packets.
int32_t check_tree_args(int32_t dev, int32_t num_nodes, int32_t num_leaf_records, bool null_pointer) {
    if (num_nodes < 1 || num_leaf_records < 1) return RODENT_BUILD_ERR_NUM_NODES;
    if (null_pointer) return RODENT_BUILD_ERR_NULL;
    return set_device(dev) ? RODENT_BUILD_OK : RODENT_BUILD_ERR_DEVICE;
}

// The argument checks of the refit entries (the builders' own, in their order).
int32_t check_refit_args(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                         const void* nodes, int32_t num_nodes, const void* tris, int32_t num_leaf_records, const void* scratch,
                         const int32_t* info_dev) {
    if (bad_num_tris(num_tris)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    return check_tree_args(dev, num_nodes, num_leaf_records, !vertices || !indices || !nodes || !tris || !scratch || !info_dev);
}

// The collapse after its argument checks: info words and record marks zeroed, parent slots set to -1, then the kernels of
// build_collapse.h: a fixed list of launches whatever the tree.  Limited: with a stack limit (`limit` > 0), one launch more.
template <class Node, bool Limited>
int32_t launch_collapse(int limit, const Node2* nodes, int num_nodes, const Tri1* tris, int num_bvh_tris, Node* wide_nodes, Tri4* packets,
                        void* scratch, int32_t* info_dev, void* stream_) {
    constexpr int N = kArity<Node>;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const CollapseScratch s = carve_collapse(static_cast<char*>(scratch), num_nodes, num_bvh_tris, Limited);
    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess
        || hipMemsetAsync(s.parent, 0xFF, 4 * (size_t)num_nodes, stream) != hipSuccess
        || hipMemsetAsync(s.mark, 0, 4 * (size_t)num_bvh_tris, stream) != hipSuccess)
        return RODENT_BUILD_ERR_LAUNCH;
    const Collapse c{nodes, num_nodes, tris, num_bvh_tris, s.parent, s.small, s.small_first, s.root, s.mark, s.wide_id, s.packet_id,
                     info_dev, s.height, s.above, Limited ? limit : 0};
    const int nb = blocks_for(num_nodes), tb = blocks_for(num_bvh_tris);
    hipLaunchKernelGGL(k_refit_links, dim3(nb), dim3(kBlock), 0, stream, nodes, num_nodes, num_bvh_tris, s.parent, s.arrivals, info_dev);
    hipLaunchKernelGGL(k_collapse_small, dim3(nb), dim3(kBlock), 0, stream, c);
    if (Limited) hipLaunchKernelGGL(k_collapse_height, dim3(nb), dim3(kBlock), 0, stream, c);
    hipLaunchKernelGGL((k_collapse_flags<N, Limited>), dim3(nb), dim3(kBlock), 0, stream, c);
    hipLaunchKernelGGL(k_collapse_totals, dim3(nb), dim3(kBlock), 0, stream, s.root, num_nodes, s.nodetot);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.nodetot, nb, info_dev + kInfoWideNodes);
    hipLaunchKernelGGL(k_collapse_ids, dim3(nb), dim3(kBlock), 0, stream, s.root, num_nodes, s.nodetot, s.wide_id);
    hipLaunchKernelGGL(k_collapse_totals, dim3(tb), dim3(kBlock), 0, stream, s.mark, num_bvh_tris, s.rectot);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.rectot, tb, info_dev + kInfoPackets);
    hipLaunchKernelGGL(k_collapse_ids, dim3(tb), dim3(kBlock), 0, stream, s.mark, num_bvh_tris, s.rectot, s.packet_id);
    hipLaunchKernelGGL(k_collapse_packets, dim3(tb), dim3(kBlock), 0, stream, c, packets);
    hipLaunchKernelGGL((k_collapse_nodes<Node, Limited>), dim3(nb), dim3(kBlock), 0, stream, c, wide_nodes);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

template <class Node>
int32_t launch_collapse(int limit, const Node2* nodes, int num_nodes, const Tri1* tris, int num_bvh_tris, void* wide_nodes, Tri4* packets,
                        void* scratch, int32_t* info_dev, void* stream) {
    Node* wide = static_cast<Node*>(wide_nodes);
    return limit > 0 ? launch_collapse<Node, true>(limit, nodes, num_nodes, tris, num_bvh_tris, wide, packets, scratch, info_dev, stream)
                     : launch_collapse<Node, false>(0, nodes, num_nodes, tris, num_bvh_tris, wide, packets, scratch, info_dev, stream);
}

// Every collapse entry: stack_limit = 0 is the collapse without a limit.
int32_t collapse(int32_t dev, int32_t width, int32_t stack_limit, const Node2* nodes, int32_t num_nodes, const Tri1* tris,
                 int32_t num_bvh_tris, void* wide_nodes, Tri4* packets, void* scratch, int32_t* info_dev, void* stream) {
    if (width != 4 && width != 8) return RODENT_BUILD_ERR_WIDTH;
    if (stack_limit < 0 || stack_limit > RODENT_BUILD_MAX_STACK_LIMIT) return RODENT_BUILD_ERR_STACK_LIMIT;
    const int32_t rc = check_tree_args(dev, num_nodes, num_bvh_tris, !nodes || !tris || !wide_nodes || !packets || !scratch || !info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return width == 4
        ? launch_collapse<Node4>(stack_limit, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, stream)
        : launch_collapse<Node8>(stack_limit, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, stream);
}

template <class Node>
int32_t refit_wide(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris, Node* nodes,
                   int32_t num_nodes, Tri4* tris, int32_t num_packets, void* scratch, int32_t* info_dev, void* stream) {
    const int32_t rc = check_refit_args(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch,
                                        info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_refit_wide(vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch, info_dev, stream);
}

// The sync forms after their own checks: scratch and `words` info words in one allocation, the entry (`build(scratch, info_dev)`) on
// the null stream, the info words copied to `info`; RODENT_BUILD_ERR_INPUT when the device raised a flag.
template <class Build>
int32_t build_sync(int32_t dev, int64_t scratch_bytes, int words, int32_t* info, Build build) {
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    void* scratch = nullptr;
    if (hipMalloc(&scratch, (size_t)scratch_bytes + 4 * words) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    int32_t* info_dev = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + scratch_bytes);
    int32_t rc = build(scratch, info_dev);
    int32_t host[RODENT_BUILD_SPLIT_INFO_WORDS] = {};
    if (rc == RODENT_BUILD_OK && hipMemcpy(host, info_dev, 4 * (size_t)words, hipMemcpyDeviceToHost) != hipSuccess)
        rc = RODENT_BUILD_ERR_LAUNCH;
    (void)hipFree(scratch);
    if (info) std::copy(host, host + words, info);
    if (rc == RODENT_BUILD_OK && host[kInfoFlags]) rc = RODENT_BUILD_ERR_INPUT;
    return rc;
}

// The refits' sync forms: build_sync around `refit(scratch, info_dev)`, and RODENT_BUILD_ERR_INPUT too when a node stayed incomplete.
template <class Refit>
int32_t refit_sync(int32_t dev, int64_t scratch_bytes, int32_t num_nodes, int32_t* info, Refit refit) {
    if (scratch_bytes < 0) return RODENT_BUILD_ERR_NUM_NODES;
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    int32_t rc = build_sync(dev, scratch_bytes, RODENT_BUILD_INFO_WORDS, words, refit);
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    if (rc == RODENT_BUILD_OK && words[kInfoRefitNodes] != num_nodes) rc = RODENT_BUILD_ERR_INPUT;    // a malformed topology
    return rc;
}

// The TLAS entries, static and motion: the argument checks in the header's order, then the launch list.
template <class ObjNode, class Desc, class Rec>
int32_t build_tlas(int32_t dev, const ObjNode* nodes, const RodentObject* objects, int32_t num_objects, const Desc* descs,
                   int32_t num_instances, int32_t max_leaf, Node2* tlas_nodes, Rec* instances, void* scratch, int32_t* info_dev,
                   void* stream) {
    if (num_instances < 1 || num_instances > RODENT_TLAS_MAX_INSTANCES) return RODENT_TLAS_ERR_NUM_INSTANCES;
    if (max_leaf < 1 || max_leaf > RODENT_BUILD_MAX_LEAF) return RODENT_BUILD_ERR_MAX_LEAF;
    if (num_objects < 1) return RODENT_TLAS_ERR_NUM_OBJECTS;
    if (!nodes || !objects || !descs || !tlas_nodes || !instances || !scratch || !info_dev) return RODENT_BUILD_ERR_NULL;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    return launch_tlas(nodes, objects, num_objects, descs, num_instances, max_leaf, tlas_nodes, instances, scratch, info_dev, stream);
}

template <class ObjNode, class Desc, class Rec>
int32_t build_tlas_sync(int32_t dev, int64_t bytes, const ObjNode* nodes, const RodentObject* objects, int32_t num_objects,
                        const Desc* descs, int32_t num_instances, int32_t max_leaf, Node2* tlas_nodes, Rec* instances, int32_t* info) {
    if (bytes < 0) return RODENT_TLAS_ERR_NUM_INSTANCES;
    if (max_leaf < 1 || max_leaf > RODENT_BUILD_MAX_LEAF) return RODENT_BUILD_ERR_MAX_LEAF;
    return build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return build_tlas(dev, nodes, objects, num_objects, descs, num_instances, max_leaf, tlas_nodes, instances, scratch, info_dev,
                          nullptr);
    });
}

} // namespace

extern "C" {

int64_t rodent_hip_build_scratch_bytes(int32_t num_tris) {
    if (bad_num_tris(num_tris)) return -1;
    return (int64_t)carve(nullptr, num_tris).bytes;
}

int32_t rodent_hip_build_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev,
                                   void* stream) {
    const int32_t rc = check_args(dev, vertices, num_vertices, indices, num_tris, max_leaf, nodes, tris, scratch, info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    const RodentBuildOptions opt{max_leaf, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    return launch_build(vertices, num_vertices, indices, num_tris, opt, nullptr, nullptr, nodes, tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, int32_t* info) {
    const int64_t bytes = rodent_hip_build_scratch_bytes(num_tris);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_TRIS;
    if (max_leaf < 1 || max_leaf > 8) return RODENT_BUILD_ERR_MAX_LEAF;
    return build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_bvh2_tri1(dev, vertices, num_vertices, indices, num_tris, max_leaf, nodes, tris, scratch, info_dev,
                                          nullptr);
    });
}

int64_t rodent_hip_build_opt_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt) {
    if (bad_num_tris(num_tris) || check_options(opt) != RODENT_BUILD_OK) return -1;
    return (int64_t)carve(nullptr, num_tris, opt->treelet_passes > 0).bytes;
}

int32_t rodent_hip_build_bvh2_tri1_opt(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                       int32_t num_tris, const struct RodentBuildOptions* opt, struct Node2* nodes, struct Tri1* tris,
                                       void* scratch, int32_t* info_dev, void* stream) {
    int32_t rc = check_options(opt);
    if (rc == RODENT_BUILD_OK)
        rc = check_args(dev, vertices, num_vertices, indices, num_tris, opt->max_leaf, nodes, tris, scratch, info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    RodentBuildOptions o = *opt;
    if (num_tris == 1) o.treelet_passes = 0;          // nothing to restructure or collapse: the LBVH, byte for byte
    return launch_build(vertices, num_vertices, indices, num_tris, o, nullptr, nullptr, nodes, tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_bvh2_tri1_opt_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                            int32_t num_tris, const struct RodentBuildOptions* opt, struct Node2* nodes,
                                            struct Tri1* tris, int32_t* info) {
    const int32_t rc = check_options(opt);
    if (rc != RODENT_BUILD_OK) return rc;
    const int64_t bytes = rodent_hip_build_opt_scratch_bytes(num_tris, opt);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_TRIS;
    return build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_bvh2_tri1_opt(dev, vertices, num_vertices, indices, num_tris, opt, nodes, tris, scratch, info_dev,
                                              nullptr);
    });
}

int64_t rodent_hip_build_split_max_refs(int32_t num_tris, const struct RodentSplitOptions* split) {
    if (bad_num_tris(num_tris) || check_split(split) != RODENT_BUILD_OK) return -1;
    return split_max_refs(num_tris, split);
}

int64_t rodent_hip_build_split_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt,
                                             const struct RodentSplitOptions* split) {
    if (bad_num_tris(num_tris) || check_options(opt) != RODENT_BUILD_OK || check_split(split) != RODENT_BUILD_OK) return -1;
    const int refs = (int)split_max_refs(num_tris, split);
    return (int64_t)(carve(nullptr, refs, opt->treelet_passes > 0).bytes + carve_split(nullptr, num_tris, refs).bytes);
}

int32_t rodent_hip_build_bvh2_tri1_split(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                         int32_t num_tris, const struct RodentBuildOptions* opt, const struct RodentSplitOptions* split,
                                         struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev, void* stream) {
    int32_t rc = check_options(opt);
    if (rc == RODENT_BUILD_OK) rc = check_split(split);
    if (rc == RODENT_BUILD_OK)
        rc = check_args(dev, vertices, num_vertices, indices, num_tris, opt->max_leaf, nodes, tris, scratch, info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_build(vertices, num_vertices, indices, num_tris, *opt, split, nullptr, nodes, tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_bvh2_tri1_split_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                              int32_t num_tris, const struct RodentBuildOptions* opt,
                                              const struct RodentSplitOptions* split, struct Node2* nodes, struct Tri1* tris,
                                              int32_t* info) {
    int32_t rc = check_options(opt);
    if (rc == RODENT_BUILD_OK) rc = check_split(split);
    if (rc != RODENT_BUILD_OK) return rc;
    const int64_t bytes = rodent_hip_build_split_scratch_bytes(num_tris, opt, split);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_TRIS;
    return build_sync(dev, bytes, RODENT_BUILD_SPLIT_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_bvh2_tri1_split(dev, vertices, num_vertices, indices, num_tris, opt, split, nodes, tris, scratch,
                                                info_dev, nullptr);
    });
}

int64_t rodent_hip_build_ploc_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt,
                                            const struct RodentSplitOptions* split, const struct RodentPlocOptions* ploc) {
    if (bad_num_tris(num_tris) || check_options(opt) != RODENT_BUILD_OK || (split && check_split(split) != RODENT_BUILD_OK)
        || check_ploc(ploc, opt, split, num_tris) != RODENT_BUILD_OK)
        return -1;
    const int refs = split ? (int)split_max_refs(num_tris, split) : num_tris;
    return (int64_t)(carve(nullptr, refs, true).bytes + (split ? carve_split(nullptr, num_tris, refs).bytes : 0)
                     + carve_ploc(nullptr, refs).bytes);
}

int32_t rodent_hip_build_bvh2_tri1_ploc(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, const struct RodentBuildOptions* opt, const struct RodentSplitOptions* split,
                                        const struct RodentPlocOptions* ploc, struct Node2* nodes, struct Tri1* tris, void* scratch,
                                        int32_t* info_dev, void* stream) {
    int32_t rc = check_options(opt);
    if (rc == RODENT_BUILD_OK && split) rc = check_split(split);
    if (rc == RODENT_BUILD_OK) rc = check_ploc(ploc, opt, split, num_tris);
    if (rc == RODENT_BUILD_OK)
        rc = check_args(dev, vertices, num_vertices, indices, num_tris, opt->max_leaf, nodes, tris, scratch, info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_build(vertices, num_vertices, indices, num_tris, *opt, split, ploc, nodes, tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_bvh2_tri1_ploc_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                             int32_t num_tris, const struct RodentBuildOptions* opt,
                                             const struct RodentSplitOptions* split, const struct RodentPlocOptions* ploc,
                                             struct Node2* nodes, struct Tri1* tris, int32_t* info) {
    int32_t rc = check_options(opt);
    if (rc == RODENT_BUILD_OK && split) rc = check_split(split);
    if (rc == RODENT_BUILD_OK) rc = check_ploc(ploc, opt, split, num_tris);
    if (rc != RODENT_BUILD_OK) return rc;
    const int64_t bytes = rodent_hip_build_ploc_scratch_bytes(num_tris, opt, split, ploc);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_TRIS;
    return build_sync(dev, bytes, RODENT_BUILD_SPLIT_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_bvh2_tri1_ploc(dev, vertices, num_vertices, indices, num_tris, opt, split, ploc, nodes, tris, scratch,
                                               info_dev, nullptr);
    });
}

int64_t rodent_hip_refit_scratch_bytes(int32_t num_nodes, int32_t num_bvh_tris) {
    if (num_nodes < 1 || num_bvh_tris < 1) return -1;
    return (int64_t)carve_refit(nullptr, num_nodes, num_bvh_tris).bytes;
}

int32_t rodent_hip_refit_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node2* nodes, int32_t num_nodes, struct Tri1* tris, int32_t num_bvh_tris, void* scratch,
                                   int32_t* info_dev, void* stream) {
    const int32_t rc = check_refit_args(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, scratch,
                                        info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_refit(vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, scratch, info_dev, stream);
}

int32_t rodent_hip_refit_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node2* nodes, int32_t num_nodes, struct Tri1* tris,
                                        int32_t num_bvh_tris, int32_t* info) {
    return refit_sync(dev, rodent_hip_refit_scratch_bytes(num_nodes, num_bvh_tris), num_nodes, info,
                      [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_refit_bvh2_tri1(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, scratch,
                                          info_dev, nullptr);
    });
}

int32_t rodent_hip_fuse_motion_bvh2_tri1(int32_t dev, const struct Node2* nodes0, const struct Tri1* tris0, const struct Node2* nodes1,
                                         const struct Tri1* tris1, int32_t num_nodes, int32_t num_bvh_tris,
                                         struct RodentMotionNode2* motion_nodes, struct RodentMotionTri1* motion_tris, int32_t* info_dev,
                                         void* stream) {
    const int32_t rc = check_tree_args(dev, num_nodes, num_bvh_tris,
                                       !nodes0 || !tris0 || !nodes1 || !tris1 || !motion_nodes || !motion_tris || !info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_fuse_motion(nodes0, tris0, nodes1, tris1, num_nodes, num_bvh_tris, motion_nodes, motion_tris, nullptr, info_dev, stream);
}

int64_t rodent_hip_motion_bvh2_scratch_bytes(int32_t num_nodes, int32_t num_bvh_tris) {
    if (num_nodes < 1 || num_bvh_tris < 1) return -1;
    return (int64_t)carve_motion(nullptr, num_nodes, num_bvh_tris).bytes;
}

int32_t rodent_hip_build_motion_bvh2_tri1(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                          const int32_t* indices, int32_t num_tris, const struct Node2* nodes, int32_t num_nodes,
                                          const struct Tri1* tris, int32_t num_bvh_tris, struct RodentMotionNode2* motion_nodes,
                                          struct RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream) {
    // check_refit_args' order, with this entry's pointers
    if (bad_num_tris(num_tris)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    const int32_t rc = check_tree_args(dev, num_nodes, num_bvh_tris, !vertices0 || !vertices1 || !indices || !nodes || !tris || !motion_nodes
                                                                         || !motion_tris || !scratch || !info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    return launch_motion_build(vertices0, vertices1, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, motion_nodes,
                               motion_tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_motion_bvh2_tri1_sync(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                               const int32_t* indices, int32_t num_tris, const struct Node2* nodes, int32_t num_nodes,
                                               const struct Tri1* tris, int32_t num_bvh_tris, struct RodentMotionNode2* motion_nodes,
                                               struct RodentMotionTri1* motion_tris, int32_t* info) {
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    int32_t rc = refit_sync(dev, rodent_hip_motion_bvh2_scratch_bytes(num_nodes, num_bvh_tris), num_nodes, words,
                            [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_motion_bvh2_tri1(dev, vertices0, vertices1, num_vertices, indices, num_tris, nodes, num_nodes, tris,
                                                 num_bvh_tris, motion_nodes, motion_tris, scratch, info_dev, nullptr);
    });
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    if (rc == RODENT_BUILD_OK && words[3] != num_nodes) rc = RODENT_BUILD_ERR_INPUT;      // key 1's count (refit_sync checked key 0's)
    return rc;
}

int64_t rodent_hip_refit_wide_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_packets) {
    if ((width != 4 && width != 8) || num_nodes < 1 || num_packets < 1) return -1;
    return (int64_t)carve_refit(nullptr, num_nodes, num_packets).bytes;
}

int32_t rodent_hip_refit_bvh4_tri4(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node4* nodes, int32_t num_nodes, struct Tri4* tris, int32_t num_packets, void* scratch,
                                   int32_t* info_dev, void* stream) {
    return refit_wide(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch, info_dev, stream);
}

int32_t rodent_hip_refit_bvh8_tri4(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node8* nodes, int32_t num_nodes, struct Tri4* tris, int32_t num_packets, void* scratch,
                                   int32_t* info_dev, void* stream) {
    return refit_wide(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch, info_dev, stream);
}

int32_t rodent_hip_refit_bvh4_tri4_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node4* nodes, int32_t num_nodes, struct Tri4* tris,
                                        int32_t num_packets, int32_t* info) {
    return refit_sync(dev, rodent_hip_refit_wide_scratch_bytes(4, num_nodes, num_packets), num_nodes, info,
                      [&](void* scratch, int32_t* info_dev) {
        return refit_wide(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch, info_dev, nullptr);
    });
}

int32_t rodent_hip_refit_bvh8_tri4_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node8* nodes, int32_t num_nodes, struct Tri4* tris,
                                        int32_t num_packets, int32_t* info) {
    return refit_sync(dev, rodent_hip_refit_wide_scratch_bytes(8, num_nodes, num_packets), num_nodes, info,
                      [&](void* scratch, int32_t* info_dev) {
        return refit_wide(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_packets, scratch, info_dev, nullptr);
    });
}

int64_t rodent_hip_collapse_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_bvh_tris) {
    if ((width != 4 && width != 8) || num_nodes < 1 || num_bvh_tris < 1) return -1;
    return (int64_t)carve_collapse(nullptr, num_nodes, num_bvh_tris, false).bytes;
}

int64_t rodent_hip_collapse_bounded_scratch_bytes(int32_t width, int32_t num_nodes, int32_t num_bvh_tris) {
    if ((width != 4 && width != 8) || num_nodes < 1 || num_bvh_tris < 1) return -1;
    return (int64_t)carve_collapse(nullptr, num_nodes, num_bvh_tris, true).bytes;
}

int32_t rodent_hip_collapse_bvh2_tri1(int32_t dev, int32_t width, const struct Node2* nodes, int32_t num_nodes, const struct Tri1* tris,
                                      int32_t num_bvh_tris, void* wide_nodes, struct Tri4* packets, void* scratch, int32_t* info_dev,
                                      void* stream) {
    return collapse(dev, width, 0, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, stream);
}

int32_t rodent_hip_collapse_bvh2_tri1_sync(int32_t dev, int32_t width, const struct Node2* nodes, int32_t num_nodes,
                                           const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes, struct Tri4* packets,
                                           int32_t* info) {
    if (width != 4 && width != 8) return RODENT_BUILD_ERR_WIDTH;
    const int64_t bytes = rodent_hip_collapse_scratch_bytes(width, num_nodes, num_bvh_tris);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_NODES;
    return build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return collapse(dev, width, 0, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, nullptr);
    });
}

int32_t rodent_hip_collapse_bvh2_tri1_bounded(int32_t dev, int32_t width, int32_t stack_limit, const struct Node2* nodes,
                                              int32_t num_nodes, const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes,
                                              struct Tri4* packets, void* scratch, int32_t* info_dev, void* stream) {
    return collapse(dev, width, stack_limit, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, stream);
}

int32_t rodent_hip_collapse_bvh2_tri1_bounded_sync(int32_t dev, int32_t width, int32_t stack_limit, const struct Node2* nodes,
                                                   int32_t num_nodes, const struct Tri1* tris, int32_t num_bvh_tris, void* wide_nodes,
                                                   struct Tri4* packets, int32_t* info) {
    if (width != 4 && width != 8) return RODENT_BUILD_ERR_WIDTH;
    if (stack_limit < 0 || stack_limit > RODENT_BUILD_MAX_STACK_LIMIT) return RODENT_BUILD_ERR_STACK_LIMIT;
    const int64_t bytes = rodent_hip_collapse_bounded_scratch_bytes(width, num_nodes, num_bvh_tris);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_NODES;
    return build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, info, [&](void* scratch, int32_t* info_dev) {
        return collapse(dev, width, stack_limit, nodes, num_nodes, tris, num_bvh_tris, wide_nodes, packets, scratch, info_dev, nullptr);
    });
}

int64_t rodent_hip_tlas_scratch_bytes(int32_t num_instances) {
    if (num_instances < 1 || num_instances > RODENT_TLAS_MAX_INSTANCES) return -1;
    return (int64_t)(carve(nullptr, num_instances).bytes + carve_tlas<RodentInstance>(nullptr, num_instances).bytes);
}

int64_t rodent_hip_motion_tlas_scratch_bytes(int32_t num_instances) {
    if (num_instances < 1 || num_instances > RODENT_TLAS_MAX_INSTANCES) return -1;
    return (int64_t)(carve(nullptr, num_instances).bytes + carve_tlas<RodentMotionInstance>(nullptr, num_instances).bytes);
}

int32_t rodent_hip_build_tlas(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                              const struct RodentInstanceDesc* descs, int32_t num_instances, int32_t max_leaf, struct Node2* tlas_nodes,
                              struct RodentInstance* instances, void* scratch, int32_t* info_dev, void* stream) {
    return build_tlas(dev, nodes, objects, num_objects, descs, num_instances, max_leaf, tlas_nodes, instances, scratch, info_dev, stream);
}

int32_t rodent_hip_build_tlas_sync(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                   const struct RodentInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                   struct Node2* tlas_nodes, struct RodentInstance* instances, int32_t* info) {
    return build_tlas_sync(dev, rodent_hip_tlas_scratch_bytes(num_instances), nodes, objects, num_objects, descs, num_instances, max_leaf,
                           tlas_nodes, instances, info);
}

int32_t rodent_hip_build_motion_tlas(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                     const struct RodentMotionInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                     struct Node2* tlas_nodes, struct RodentMotionInstance* instances, void* scratch, int32_t* info_dev,
                                     void* stream) {
    return build_tlas(dev, nodes, objects, num_objects, descs, num_instances, max_leaf, tlas_nodes, instances, scratch, info_dev, stream);
}

int32_t rodent_hip_build_motion_tlas_sync(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                          const struct RodentMotionInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                          struct Node2* tlas_nodes, struct RodentMotionInstance* instances, int32_t* info) {
    return build_tlas_sync(dev, rodent_hip_motion_tlas_scratch_bytes(num_instances), nodes, objects, num_objects, descs, num_instances,
                           max_leaf, tlas_nodes, instances, info);
}

int64_t rodent_hip_refit_objects_plan(const struct RodentObject* objects, int32_t num_objects, const int32_t* listed,
                                      const int32_t* first_tri, const int32_t* num_tris, int32_t num_listed,
                                      struct RodentRefitRange* ranges, int32_t* totals) {
    if (!objects || !listed || !first_tri || !num_tris || !ranges || !totals || num_objects < 1 || num_listed < 1) return -1;
    int64_t nodes = 0, recs = 0;
    for (int32_t k = 0; k < num_listed; k++) {
        const bool known = listed[k] >= 0 && listed[k] < num_objects;
        ranges[k] = RodentRefitRange{listed[k], first_tri[k], num_tris[k], (int32_t)nodes, (int32_t)recs, {0, 0, 0}};
        nodes += known ? std::max(objects[listed[k]].num_nodes, 0) : 0;
        recs += known ? std::max(objects[listed[k]].num_tris, 0) : 0;
        if (nodes > INT32_MAX || recs > INT32_MAX) return -1;
    }
    totals[0] = (int32_t)nodes; totals[1] = (int32_t)recs;
    return (int64_t)std::max<size_t>(carve_refit(nullptr, (int)nodes, (int)recs).bytes, 256);
}

int32_t rodent_hip_refit_objects(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                 struct Node2* nodes, struct Tri1* tris, const struct RodentObject* objects, int32_t num_objects,
                                 const struct RodentRefitRange* ranges, int32_t num_listed, int32_t total_nodes, int32_t total_recs,
                                 void* scratch, int32_t* info_dev, void* stream) {
    if (bad_num_tris(num_rows)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (num_objects < 1) return RODENT_TLAS_ERR_NUM_OBJECTS;
    if (num_listed < 1 || total_nodes < 0 || total_recs < 0) return RODENT_BUILD_ERR_NUM_NODES;
    if (!vertices || !indices || !nodes || !tris || !objects || !ranges || !scratch || !info_dev) return RODENT_BUILD_ERR_NULL;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    const ForestArgs a{objects, ranges, num_objects, num_listed, total_nodes, total_recs, num_rows};
    return launch_refit_objects(vertices, num_vertices, indices, nodes, tris, a, scratch, info_dev, stream);
}

// RODENT_BUILD_ERR_NUM_NODES of rodent_hip_build_motion_objects: rodent_hip_refit_objects' class and the packed arrays' counts.
static bool bad_motion_objects_counts(int32_t num_listed, int32_t total_nodes, int32_t total_recs, int32_t num_nodes, int32_t num_recs) {
    return num_listed < 1 || total_nodes < 0 || total_recs < 0 || num_nodes < 1 || num_recs < 1 || total_nodes > num_nodes
        || total_recs > num_recs;
}

int64_t rodent_hip_motion_objects_scratch_bytes(int32_t num_nodes, int32_t num_recs, int64_t refit_bytes) {
    if (num_nodes < 1 || num_recs < 1 || refit_bytes < 0) return -1;
    return (int64_t)carve_motion(nullptr, num_nodes, num_recs, (size_t)refit_bytes).bytes;
}

int32_t rodent_hip_build_motion_objects(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                        const int32_t* indices, int32_t num_rows, const struct Node2* nodes, int32_t num_nodes,
                                        const struct Tri1* tris, int32_t num_recs, const struct RodentObject* objects,
                                        int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed,
                                        int32_t total_nodes, int32_t total_recs, struct RodentMotionNode2* motion_nodes,
                                        struct RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream) {
    // rodent_hip_refit_objects' order, with this entry's counts and pointers
    if (bad_num_tris(num_rows)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (num_objects < 1) return RODENT_TLAS_ERR_NUM_OBJECTS;
    if (bad_motion_objects_counts(num_listed, total_nodes, total_recs, num_nodes, num_recs)) return RODENT_BUILD_ERR_NUM_NODES;
    if (!vertices0 || !vertices1 || !indices || !nodes || !tris || !objects || !ranges || !motion_nodes || !motion_tris || !scratch
        || !info_dev)
        return RODENT_BUILD_ERR_NULL;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    const ForestArgs a{objects, ranges, num_objects, num_listed, total_nodes, total_recs, num_rows};
    return launch_motion_objects(vertices0, vertices1, num_vertices, indices, nodes, num_nodes, tris, num_recs, a, motion_nodes,
                                 motion_tris, scratch, info_dev, stream);
}

int32_t rodent_hip_build_motion_objects_sync(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                             const int32_t* indices, int32_t num_rows, const struct Node2* nodes, int32_t num_nodes,
                                             const struct Tri1* tris, int32_t num_recs, const struct RodentObject* objects,
                                             int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed,
                                             int32_t total_nodes, int32_t total_recs, struct RodentMotionNode2* motion_nodes,
                                             struct RodentMotionTri1* motion_tris, int32_t* info) {
    if (bad_motion_objects_counts(num_listed, total_nodes, total_recs, num_nodes, num_recs)) return RODENT_BUILD_ERR_NUM_NODES;
    const int64_t refit_bytes = (int64_t)std::max<size_t>(carve_refit(nullptr, total_nodes, total_recs).bytes, 256);
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    int32_t rc = refit_sync(dev, rodent_hip_motion_objects_scratch_bytes(num_nodes, num_recs, refit_bytes), total_nodes, words,
                            [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_build_motion_objects(dev, vertices0, vertices1, num_vertices, indices, num_rows, nodes, num_nodes, tris,
                                               num_recs, objects, num_objects, ranges, num_listed, total_nodes, total_recs, motion_nodes,
                                               motion_tris, scratch, info_dev, nullptr);
    });
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    if (rc == RODENT_BUILD_OK && words[3] != total_nodes) rc = RODENT_BUILD_ERR_INPUT;    // key 1's count (refit_sync checked key 0's)
    return rc;
}

int32_t rodent_hip_build_motion_tlas_motion_objects(int32_t dev, const struct RodentMotionNode2* nodes,
                                                    const struct RodentObject* objects, int32_t num_objects,
                                                    const struct RodentMotionInstanceDesc* descs, int32_t num_instances,
                                                    int32_t max_leaf, struct Node2* tlas_nodes, struct RodentMotionInstance* instances,
                                                    void* scratch, int32_t* info_dev, void* stream) {
    return build_tlas(dev, nodes, objects, num_objects, descs, num_instances, max_leaf, tlas_nodes, instances, scratch, info_dev, stream);
}

int32_t rodent_hip_build_motion_tlas_motion_objects_sync(int32_t dev, const struct RodentMotionNode2* nodes,
                                                         const struct RodentObject* objects, int32_t num_objects,
                                                         const struct RodentMotionInstanceDesc* descs, int32_t num_instances,
                                                         int32_t max_leaf, struct Node2* tlas_nodes,
                                                         struct RodentMotionInstance* instances, int32_t* info) {
    return build_tlas_sync(dev, rodent_hip_motion_tlas_scratch_bytes(num_instances), nodes, objects, num_objects, descs, num_instances,
                           max_leaf, tlas_nodes, instances, info);
}

int64_t rodent_hip_build_objects_plan(const int32_t* listed, const int32_t* first_tri, const int32_t* num_tris, int32_t num_listed,
                                      struct RodentRefitRange* ranges, int32_t* totals) {
    if (!listed || !first_tri || !num_tris || !ranges || !totals || num_listed < 1 || num_listed > RODENT_BUILD_OBJECTS_MAX_LISTED)
        return -1;
    int64_t tris = 0;
    for (int32_t k = 0; k < num_listed; k++) {
        if (num_tris[k] < 1) return -1;
        ranges[k] = RodentRefitRange{listed[k], first_tri[k], num_tris[k], (int32_t)tris, (int32_t)tris, {0, 0, 0}};
        tris += num_tris[k];
        if (tris > kMaxTris) return -1;
    }
    totals[0] = (int32_t)tris;
    return (int64_t)carve_forest_build(nullptr, (int)tris, num_listed).bytes;
}

int32_t rodent_hip_build_objects(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                 int32_t max_leaf, int32_t mode, struct Node2* nodes, struct Tri1* tris, struct RodentObject* objects,
                                 int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed, int32_t total_tris,
                                 void* scratch, int32_t* object_info, int32_t* info_dev, void* stream) {
    if (bad_num_tris(num_rows)) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (num_objects < 1) return RODENT_TLAS_ERR_NUM_OBJECTS;
    if (num_listed < 1 || num_listed > RODENT_BUILD_OBJECTS_MAX_LISTED || bad_num_tris(total_tris)) return RODENT_BUILD_ERR_NUM_NODES;
    if (max_leaf < 1 || max_leaf > RODENT_BUILD_MAX_LEAF) return RODENT_BUILD_ERR_MAX_LEAF;
    if (mode != RODENT_BUILD_OBJECTS_IN_PLACE && mode != RODENT_BUILD_OBJECTS_PACK) return RODENT_BUILD_ERR_INPUT;
    if (!vertices || !indices || !nodes || !tris || !objects || !ranges || !scratch || !object_info || !info_dev)
        return RODENT_BUILD_ERR_NULL;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    BuildForest a{};
    a.objects = objects; a.ranges = ranges; a.num_objects = num_objects; a.num_listed = num_listed; a.total_tris = total_tris;
    a.num_rows = num_rows; a.max_leaf = max_leaf; a.pack = mode == RODENT_BUILD_OBJECTS_PACK; a.object_info = object_info;
    a.info = info_dev;
    return launch_build_objects(vertices, num_vertices, indices, nodes, tris, a, scratch, stream);
}

int32_t rodent_hip_build_objects_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                      int32_t max_leaf, int32_t mode, struct Node2* nodes, struct Tri1* tris,
                                      struct RodentObject* objects, int32_t num_objects, const struct RodentRefitRange* ranges,
                                      int32_t num_listed, int32_t total_tris, int32_t* object_info, int32_t* info) {
    if (num_listed < 1 || num_listed > RODENT_BUILD_OBJECTS_MAX_LISTED || bad_num_tris(total_tris)) return RODENT_BUILD_ERR_NUM_NODES;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    const size_t scratch_bytes = carve_forest_build(nullptr, total_tris, num_listed).bytes, words = 4 * (size_t)num_listed;
    char* scratch = nullptr;
    if (hipMalloc(&scratch, scratch_bytes + 4 * (words + RODENT_BUILD_INFO_WORDS)) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    int32_t* object_info_dev = reinterpret_cast<int32_t*>(scratch + scratch_bytes);
    int32_t* info_dev = object_info_dev + words;
    int32_t rc = rodent_hip_build_objects(dev, vertices, num_vertices, indices, num_rows, max_leaf, mode, nodes, tris, objects,
                                          num_objects, ranges, num_listed, total_tris, scratch, object_info_dev, info_dev, nullptr);
    int32_t host[RODENT_BUILD_INFO_WORDS] = {};
    if (rc == RODENT_BUILD_OK && (hipMemcpy(host, info_dev, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess
                                  || (object_info && hipMemcpy(object_info, object_info_dev, 4 * words, hipMemcpyDeviceToHost) != hipSuccess)))
        rc = RODENT_BUILD_ERR_LAUNCH;
    (void)hipFree(scratch);
    if (info) std::copy(host, host + RODENT_BUILD_INFO_WORDS, info);
    if (rc == RODENT_BUILD_OK && host[kInfoFlags]) rc = RODENT_BUILD_ERR_INPUT;
    return rc;
}

} // extern "C"
