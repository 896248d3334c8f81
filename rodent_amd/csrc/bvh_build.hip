// bvh_build.hip -- BVH builder on the device writing BVH2 / Tri1 in the layout of include/rodent_traversal.h: a linear BVH (Morton
// codes + Karras 2012 hierarchy), optionally restructured by treelets with an SAH leaf collapse, optionally over pre-split triangles.
// C ABI: include/rodent_build.h.  CPU models of every stage, byte for byte: tests/lbvh_model.py, tests/trbvh_model.py (treelets),
// tests/split_model.py (pre-splitting).
//
// One pipeline (launch_build), all on the caller's stream, nothing allocated, no host synchronisation.  The three entry points only
// choose its options: rodent_hip_build_bvh2_tri1 the LBVH, _opt treelet_passes (0, or one triangle: the LBVH), _split the split front.
// Front, one of:
//   k_centroids      per triangle: indices checked before any vertex load, centroid sum s = (v0 + v1) + v2, per-block min / max
//   k_bounds         one block: the centroid bounds and per-axis scale = 1024 / extent (0 for an empty or non-finite extent)
// or (split) the pre-splitting stages of section 9, k_split_boxes ... k_refs, which make the n' references, then k_bounds over
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
// Split, n' is known on the device only: the tree and tail stages get grids sized for max_refs and read n' (`nref`) from info[4];
// without `nref` the host sizes them for the n triangles.
// Refit (section 11, rodent_hip_refit_bvh2_tri1): k_refit_links, k_refit_tris, k_refit_climb rewrite the boxes and Tri1 records of an
// existing hierarchy in place from moved vertices; the topology stays.  CPU model: tests/refit_model.py.
// Every value is a function of the inputs alone: min / max are exact and do not depend on the order they are taken in, the sort is
// stable, and arrival order decides only WHICH thread computes a node, never what it computes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rodent_build.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRadixItems = 16;                          // keys per thread and pass: a tile of 4096
constexpr int kRadixTile = kBlock * kRadixItems;
constexpr int kBoundsBlocks = 1024;                      // partial centroid bounds (grid-stride)
constexpr int kMaxTris = 1 << 25;
constexpr uint32_t kLastInLeaf = 0x80000000u;

enum { kInfoNodes = 0, kInfoDepth = 1, kInfoFlags = 2 };

// ---- scratch layout: one carving shared by rodent_hip_build_scratch_bytes and the launcher ------------------------------------
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
    size_t off = 0;
    const auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return p; };
    const size_t N = (size_t)n, M = (size_t)std::max(n - 1, 1);
    for (int k = 0; k < 2; k++) { s.keys[k] = (uint32_t*)take(4 * N); s.vals[k] = (uint32_t*)take(4 * N); }
    s.hist = (uint32_t*)take(4 * 256 * (size_t)radix_tiles(n));
    s.partial = (float*)take(4 * 6 * kBoundsBlocks);
    s.frame = (float*)take(4 * 8);
    s.cent = (float4*)take(16 * N);
    s.leafbox = (float*)take(4 * 6 * N);
    s.first = (int*)take(4 * M); s.last = (int*)take(4 * M); s.split = (int*)take(4 * M); s.parent = (int*)take(4 * M);
    s.leaf_parent = (int*)take(4 * N); s.height = (int*)take(4 * M); s.newidx = (int*)take(4 * M);
    s.box = (float*)take(4 * 6 * M);
    s.arrivals = (uint32_t*)take(4 * M);
    s.blockcount = (uint32_t*)take(4 * ((M + kBlock - 1) / kBlock));
    if (opt) {
        s.left = (int*)take(4 * M); s.right = (int*)take(4 * M); s.count = (int*)take(4 * M); s.emitted = (int*)take(4 * M);
        s.depth = (int*)take(4 * M); s.cost = (float*)take(4 * M);
    }
    s.bytes = off;
    return s;
}

// ---- wave64 helpers ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ uint64_t lanes_below() { return __lanemask_lt(); }

// -0 -> +0 (x + 0 is +0 for both zeros): box corners then have one bit pattern whichever of two equal zeros min / max returns
__device__ __forceinline__ float canon(float x) { return x + 0.0f; }

// The vertex triple of triangle t, each index checked before its vertex is read: an index outside [0, num_vertices) reads as the
// origin and raises kBuildBadIndex (when `info` is given), a non-finite coordinate raises kBuildNonFinite.
__device__ __forceinline__ int load_triangle(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int t,
                                             float3 v[3], int* geom, int* info) {
    const int4 ix = indices[t];
    const int id[3] = {ix.x, ix.y, ix.z};
    int flags = 0;
    for (int k = 0; k < 3; k++) {
        if ((unsigned)id[k] < (unsigned)nv) {
            const float4 p = vertices[id[k]];
            v[k] = make_float3(p.x, p.y, p.z);
            if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) flags |= RODENT_BUILD_NON_FINITE;
        } else {
            v[k] = make_float3(0.0f, 0.0f, 0.0f);
            flags |= RODENT_BUILD_BAD_INDEX;
        }
    }
    *geom = ix.w;
    if (info && flags) atomicOr(&info[kInfoFlags], flags);
    return flags;
}

// The geometry of a Tri1 record: v0, e1 = v0 - v1, e2 = v2 - v0 (k_leaves, k_emit_opt_tris and the refit write these very values).
struct TriGeometry { float3 v0, e1, e2; };
__device__ __forceinline__ TriGeometry tri1_geometry(const float3 v[3]) {
    TriGeometry g;
    g.v0 = v[0];
    g.e1 = make_float3(v[0].x - v[1].x, v[0].y - v[1].y, v[0].z - v[1].z);
    g.e2 = make_float3(v[2].x - v[0].x, v[2].y - v[0].y, v[2].z - v[0].z);
    return g;
}

// The box of a triangle's corners taken as x + 0: lo_x hi_x lo_y hi_y lo_z hi_z.
__device__ __forceinline__ void triangle_box(const float3 v[3], float* box) {
    const float c[3][3] = {{v[0].x, v[1].x, v[2].x}, {v[0].y, v[1].y, v[2].y}, {v[0].z, v[1].z, v[2].z}};
    for (int a = 0; a < 3; a++) {
        box[2 * a] = fminf(fminf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
        box[2 * a + 1] = fmaxf(fmaxf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
    }
}

// ---- 1. centroids and their bounds ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_centroids(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                      int n, float4* __restrict__ cent, float* __restrict__ partial, int* info) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        float3 v[3]; int geom;
        load_triangle(vertices, nv, indices, t, v, &geom, info);
        const float s[3] = {(v[0].x + v[1].x) + v[2].x, (v[0].y + v[1].y) + v[2].y, (v[0].z + v[1].z) + v[2].z};
        cent[t] = make_float4(s[0], s[1], s[2], 0.0f);
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], s[a]); hi[a] = fmaxf(hi[a], s[a]); }
    }
    __shared__ float red[6][kBlock];
    for (int a = 0; a < 3; a++) { red[a][threadIdx.x] = lo[a]; red[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 3; a++) {
                red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
                red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[6 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void k_bounds(const float* __restrict__ partial, int blocks, float* __restrict__ frame) {
    __shared__ float red[6][kBlock];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < blocks; b += kBlock)
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partial[6 * b + a]); hi[a] = fmaxf(hi[a], partial[6 * b + 3 + a]); }
    for (int a = 0; a < 3; a++) { red[a][threadIdx.x] = lo[a]; red[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 3; a++) {
                red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
                red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float l = red[a][0], extent = red[3 + a][0] - l;
        frame[a] = l;
        // an axis without extent (or with a non-finite one) gets cell 0 everywhere, never a division by zero
        frame[3 + a] = (extent > 0.0f && isfinite(extent)) ? __fdiv_rn(1024.0f, extent) : 0.0f;
    }
}

// ---- 2. Morton codes --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t x) {    // bit k -> bit 3k
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ __launch_bounds__(kBlock) void k_morton(const float4* __restrict__ cent, int n, const float* __restrict__ frame,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, const int* nref) {
    if (nref) n = *nref;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const float4 c = cent[t];
    const float s[3] = {c.x, c.y, c.z};
    uint32_t cell[3];
    for (int a = 0; a < 3; a++) {
        const float q = (s[a] - frame[a]) * frame[3 + a];
        cell[a] = (uint32_t)fminf(fmaxf(q, 0.0f), 1023.0f);     // fmaxf takes 0 over a NaN
    }
    keys[t] = (spread10(cell[0]) << 2) | (spread10(cell[1]) << 1) | spread10(cell[2]);
    vals[t] = (uint32_t)t;
}

// ---- 3. stable LSD radix sort, 8 bits per pass ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_radix_hist(const uint32_t* __restrict__ keys, int n, int shift, uint32_t* __restrict__ hist,
                                                       const int* nref) {
    if (nref) n = *nref;                               // tiles past n' count nothing: their digits scan to the same places
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * kRadixTile;
    for (int it = 0; it < kRadixItems; it++) {
        const int i = base + it * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// Exclusive scan of a[0, count) in place by ONE block of 1024 threads (each a contiguous run); the total goes to *total when given.
__global__ __launch_bounds__(1024) void k_scan(uint32_t* a, int count, int* total) {
    __shared__ uint32_t part[1024];
    const int per = (count + 1023) / 1024, begin = min((int)threadIdx.x * per, count), end = min(begin + per, count);
    uint32_t sum = 0;
    for (int k = begin; k < end; k++) sum += a[k];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {                // inclusive Hillis-Steele scan of the run sums
        const uint32_t add = (int)threadIdx.x >= w ? part[threadIdx.x - w] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (int k = begin; k < end; k++) { const uint32_t v = a[k]; a[k] = run; run += v; }
    if (total && threadIdx.x == 1023) *total = (int)part[1023];
}

// Scatter of one tile to the places k_scan gave its digits; inside the tile keys keep their order (wave ranks from 8 ballots, waves in
// order, 256 keys at a time), so the pass is stable.
__global__ __launch_bounds__(kBlock) void k_radix_scatter(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                          uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                          const uint32_t* __restrict__ hist, int n, int shift, const int* nref) {
    if (nref) n = *nref;
    __shared__ uint32_t running[256];
    __shared__ uint32_t wcount[kBlock / 64][256];
    const int tid = threadIdx.x, w = tid >> 6;
    running[tid] = hist[(size_t)tid * gridDim.x + blockIdx.x];
    for (int k = 0; k < kBlock / 64; k++) wcount[k][tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * kRadixTile;
    for (int it = 0; it < kRadixItems && base + it * kBlock < n; it++) {
        const int i = base + it * kBlock + tid;
        const bool valid = i < n;
        const uint32_t key = valid ? kin[i] : 0u, val = valid ? vin[i] : 0u, d = (key >> shift) & 255u;
        uint64_t same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const uint64_t ones = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? ones : ~ones;
        }
        const uint32_t rank = (uint32_t)__popcll(same & lanes_below());
        if (valid && rank == 0) wcount[w][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = running[d] + rank;
            for (int k = 0; k < w; k++) pos += wcount[k][d];
            kout[pos] = key; vout[pos] = val;
        }
        __syncthreads();
        uint32_t add = 0;
        for (int k = 0; k < kBlock / 64; k++) { add += wcount[k][tid]; wcount[k][tid] = 0; }
        running[tid] += add;
        __syncthreads();
    }
}

// ---- 4. leaves: Tri1 records and boxes in sorted order ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_leaves(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                   const uint32_t* __restrict__ order, int n, Tri1* __restrict__ tris,
                                                   float* __restrict__ leafbox, const int* nref, const int* __restrict__ reftri,
                                                   const float* __restrict__ refbox) {
    if (nref) n = *nref;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int r = (int)order[p], t = reftri ? reftri[r] : r;      // the split entry sorts references: triangle and box through them
    float3 v[3]; int geom;
    load_triangle(vertices, nv, indices, t, v, &geom, nullptr);
    const TriGeometry g = tri1_geometry(v);
    float4* out = reinterpret_cast<float4*>(tris + p);
    out[0] = make_float4(g.v0.x, g.v0.y, g.v0.z, 0.0f);
    out[1] = make_float4(g.e1.x, g.e1.y, g.e1.z, __int_as_float(geom));
    out[2] = make_float4(g.e2.x, g.e2.y, g.e2.z, __int_as_float(t));
    if (refbox) {
        for (int k = 0; k < 6; k++) leafbox[6 * (size_t)p + k] = refbox[6 * (size_t)r + k];
        return;
    }
    triangle_box(v, leafbox + 6 * (size_t)p);
}

// ---- 5. Karras hierarchy ----------------------------------------------------------------------------------------------------
// Common prefix length of sorted positions i and j; equal codes fall back to the positions themselves (32 + clz(i ^ j)), so every
// pair differs.  -1 outside [0, n).
__device__ __forceinline__ int delta(const uint32_t* __restrict__ codes, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = codes[i], b = codes[j];
    return a != b ? __clz((int)(a ^ b)) : 32 + __clz(i ^ j);
}

__global__ __launch_bounds__(kBlock) void k_karras(const uint32_t* __restrict__ codes, int n, int max_leaf, int* __restrict__ first,
                                                   int* __restrict__ last, int* __restrict__ split, int* __restrict__ parent,
                                                   int* __restrict__ leaf_parent, uint32_t* __restrict__ blockcount,
                                                   const int* nref) {
    if (nref) n = *nref;                               // blocks past n' - 1 keep nothing: their counts are 0
    const int m = n - 1, i = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false;
    if (i < m) {
        const int d = delta(codes, n, i, i + 1) > delta(codes, n, i, i - 1) ? 1 : -1;
        const int dmin = delta(codes, n, i, i - d);
        int lmax = 2;
        while (delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
        int l = 0;
        for (int t = lmax >> 1; t >= 1; t >>= 1)
            if (delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
        const int j = i + l * d, dnode = delta(codes, n, i, j);
        int s = 0, t = l;
        do {
            t = (t + 1) >> 1;
            if (delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
        } while (t > 1);
        const int g = i + s * d + min(d, 0), f = min(i, j), e = max(i, j);
        first[i] = f; last[i] = e; split[i] = g;
        if (f == g) leaf_parent[g] = i; else parent[g] = i;
        if (e == g + 1) leaf_parent[g + 1] = i; else parent[g + 1] = i;
        if (i == 0) parent[0] = -1;
        kept = e - f + 1 > max_leaf;
    }
    const int count = __syncthreads_count(kept);
    if (threadIdx.x == 0) blockcount[blockIdx.x] = (uint32_t)count;
}

__global__ __launch_bounds__(kBlock) void k_renumber(const int* __restrict__ first, const int* __restrict__ last, int m, int max_leaf,
                                                     const uint32_t* __restrict__ blockoff, int* __restrict__ newidx,
                                                     const int* nref) {
    if (nref) m = *nref - 1;
    __shared__ uint32_t wave_total[kBlock / 64];
    const int i = blockIdx.x * kBlock + threadIdx.x, w = threadIdx.x >> 6;
    const bool kept = i < m && last[i] - first[i] + 1 > max_leaf;
    const uint64_t b = __ballot(kept);
    if (lane_id() == 0) wave_total[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t idx = blockoff[blockIdx.x] + (uint32_t)__popcll(b & lanes_below());
    for (int k = 0; k < w; k++) idx += wave_total[k];
    if (i < m) newidx[i] = kept ? (int)idx : -1;
}

// ---- 6. bottom-up boxes and heights -----------------------------------------------------------------------------------------
// One thread per sorted triangle climbs from its leaf.  At each node: publish what this thread wrote (agent-scope release, its wait,
// then a relaxed agent-scope add to the node's arrival counter); the first arriver stops, the second acquires at agent scope and reads
// both children -- one of them written by the other thread, possibly on another XCD.  Nobody waits for anybody.
// height: Node2 levels under a kept node (0 for a node that becomes a leaf); the root's is the tree's depth.
__global__ __launch_bounds__(kBlock) void k_bottom_up(int n, int max_leaf, const int* __restrict__ first, const int* __restrict__ last,
                                                      const int* __restrict__ split, const int* __restrict__ parent,
                                                      const int* __restrict__ leaf_parent, const float* __restrict__ leafbox,
                                                      float* box, int* height, uint32_t* arrivals, int* info, const int* nref) {
    if (nref) n = *nref;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n || n < 2) return;
    int node = leaf_parent[p];
    while (node >= 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int f = first[node], e = last[node], g = split[node];
        const float* lb = f == g ? leafbox + 6 * (size_t)g : box + 6 * (size_t)g;
        const float* rb = e == g + 1 ? leafbox + 6 * (size_t)(g + 1) : box + 6 * (size_t)(g + 1);
        const int hl = f == g ? 0 : height[g], hr = e == g + 1 ? 0 : height[g + 1];
        for (int a = 0; a < 3; a++) {
            box[6 * (size_t)node + 2 * a] = fminf(lb[2 * a], rb[2 * a]);
            box[6 * (size_t)node + 2 * a + 1] = fmaxf(lb[2 * a + 1], rb[2 * a + 1]);
        }
        const int h = e - f + 1 > max_leaf ? 1 + max(hl, hr) : 0;
        height[node] = h;
        if (node == 0 && h > 0) info[kInfoDepth] = h;
        node = parent[node];
    }
}

// ---- 7. emission ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_bounds(float* dst, const float* b) { for (int k = 0; k < 6; k++) dst[k] = b[k]; }

__global__ __launch_bounds__(kBlock) void k_emit(int m, const int* __restrict__ first, const int* __restrict__ last,
                                                 const int* __restrict__ split, const int* __restrict__ newidx,
                                                 const float* __restrict__ leafbox, const float* __restrict__ box,
                                                 Node2* __restrict__ nodes, Tri1* __restrict__ tris, const int* nref) {
    if (nref) m = *nref - 1;                           // n' <= max_leaf: no node is kept, nothing is written
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || newidx[i] < 0) return;
    const int g = split[i];
    const int lo[2] = {first[i], g + 1}, hi[2] = {g, last[i]};       // the children's sorted ranges
    float b[12];
    int child[2];
    for (int k = 0; k < 2; k++) {
        const int c = g + k;
        const bool single = lo[k] == hi[k];
        put_bounds(b + 6 * k, single ? leafbox + 6 * (size_t)c : box + 6 * (size_t)c);
        if (!single && newidx[c] >= 0) {
            child[k] = newidx[c] + 1;
        } else {
            child[k] = ~lo[k];
            tris[hi[k]].prim_id = (int32_t)((uint32_t)tris[hi[k]].prim_id | kLastInLeaf);
        }
    }
    float4* out = reinterpret_cast<float4*>(nodes + newidx[i]);
    out[0] = make_float4(b[0], b[1], b[2], b[3]);
    out[1] = make_float4(b[4], b[5], b[6], b[7]);
    out[2] = make_float4(b[8], b[9], b[10], b[11]);
    out[3] = make_float4(__int_as_float(child[0]), __int_as_float(child[1]), 0.0f, 0.0f);
}

// n <= max_leaf: one root whose child 0 is the whole leaf; the empty slot as the host writer leaves it (+inf, -inf).  With `nref`
// (the split entry: n' on the device) it writes only when n' <= limit.
__global__ void k_emit_root(int n, const float* __restrict__ leafbox, const float* __restrict__ box, Node2* __restrict__ nodes,
                            Tri1* __restrict__ tris, int* info, const int* nref, int limit) {
    if (nref) { n = *nref; if (n > limit) return; }
    const float* b = n == 1 ? leafbox : box;
    Node2 nd;
    for (int k = 0; k < 6; k++) nd.bounds[k] = b[k];
    for (int a = 0; a < 3; a++) { nd.bounds[6 + 2 * a] = INFINITY; nd.bounds[7 + 2 * a] = -INFINITY; }
    nd.child[0] = ~0; nd.child[1] = 0; nd.pad[0] = nd.pad[1] = 0;
    nodes[0] = nd;
    tris[n - 1].prim_id = (int32_t)((uint32_t)tris[n - 1].prim_id | kLastInLeaf);
    info[kInfoNodes] = 1;
    info[kInfoDepth] = 1;
}

// ---- 8. optimisation: treelet restructuring (Karras & Aila 2013) and SAH leaf collapse --------------------------------------------
// Node ids: 0 .. m-1 inner (Karras numbering), m + p the sorted triangle p.  Arithmetic (fp32, -ffp-contract=off, in this order):
//   area A(b)   = (dx * dy + dy * dz) + dz * dx                               (half the surface area)
//   leaf cost   = (tri_cost * A) * N                                           (N triangles)
//   inner cost  = node_cost * A + (C(left) + C(right))
//   C(node)     = leaf cost when N <= max_leaf and leaf cost <= inner cost, else inner cost; a triangle's C is its leaf cost
// A node whose C is its leaf cost is "collapsed": it becomes a leaf unless an ancestor is collapsed too.
constexpr int kTreelet = 7;                              // treelet leaves
constexpr int kSubsets = 1 << kTreelet;
constexpr int kMaxDepth = 56;                            // Node2 levels the optimised tree may have
constexpr int kMaxClimb = 64;                            // bound of every walk along parent links (the depth is <= 56)

struct Opt {
    int n, m, max_leaf;
    float node_cost, tri_cost;
    int *left, *right, *parent, *leaf_parent, *count, *height, *emitted, *depth;
    float *box, *cost;
    const float* leafbox;
    const int* nref;                                     // the split entry: n' references, on the device (grids sized for max_refs)
};

// n and m from the device count when there is one; false when there is no inner node (then every optimising stage is a no-op)
__device__ __forceinline__ bool resolve(Opt& o) {
    if (o.nref) { o.n = *o.nref; o.m = o.n - 1; }
    return o.m > 0;
}

__device__ __forceinline__ float half_area(const float* b) {
    const float dx = b[1] - b[0], dy = b[3] - b[2], dz = b[5] - b[4];
    return (dx * dy + dy * dz) + dz * dx;
}
__device__ __forceinline__ const float* node_box(const Opt& o, int id) {
    return id < o.m ? o.box + 6 * (size_t)id : o.leafbox + 6 * (size_t)(id - o.m);
}
__device__ __forceinline__ int node_count(const Opt& o, int id) { return id < o.m ? o.count[id] : 1; }
__device__ __forceinline__ int node_height(const Opt& o, int id) { return id < o.m ? o.height[id] : 0; }
__device__ __forceinline__ int node_emitted(const Opt& o, int id) { return id < o.m ? o.emitted[id] : 0; }
__device__ __forceinline__ float node_cost(const Opt& o, int id) {
    return id < o.m ? o.cost[id] : (o.tri_cost * half_area(node_box(o, id))) * 1.0f;
}
__device__ __forceinline__ int parent_of(const Opt& o, int id) { return id < o.m ? o.parent[id] : o.leaf_parent[id - o.m]; }
__device__ __forceinline__ void set_parent(const Opt& o, int id, int p) {
    if (id < o.m) o.parent[id] = p; else o.leaf_parent[id - o.m] = p;
}
__device__ __forceinline__ bool valid_id(const Opt& o, int id) { return (unsigned)id < (unsigned)(o.m + o.n); }

__global__ __launch_bounds__(kBlock) void k_explicit(int m, const int* __restrict__ first, const int* __restrict__ last,
                                                     const int* __restrict__ split, int* __restrict__ left, int* __restrict__ right,
                                                     const int* nref) {
    if (nref) m = *nref - 1;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int g = split[i];
    left[i] = first[i] == g ? m + g : g;
    right[i] = last[i] == g + 1 ? m + g + 1 : g + 1;
}

// Height and cost of inner node `node` from its children l, r (area: of its box, cnt: its triangles); true when it is collapsed.
__device__ __forceinline__ bool refit(const Opt& o, int node, int l, int r, float area, int cnt) {
    const float inner = o.node_cost * area + (node_cost(o, l) + node_cost(o, r));
    const float leafc = (o.tri_cost * area) * (float)cnt;
    const bool collapse = cnt <= o.max_leaf && leafc <= inner;
    o.height[node] = 1 + max(node_height(o, l), node_height(o, r));
    o.cost[node] = collapse ? leafc : inner;
    return collapse;
}

// Box, count, height, cost and emitted-node count of every inner node, bottom-up with the hand-off of k_bottom_up.
__global__ __launch_bounds__(kBlock) void k_fit(Opt o, uint32_t* arrivals) {
    if (!resolve(o)) return;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= o.n) return;
    int node = o.leaf_parent[p];
    for (int step = 0; node >= 0 && step < kMaxClimb; step++) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int l = o.left[node], r = o.right[node];
        if (!valid_id(o, l) || !valid_id(o, r)) return;
        const float *lb = node_box(o, l), *rb = node_box(o, r);
        float b[6];
        for (int a = 0; a < 3; a++) { b[2 * a] = fminf(lb[2 * a], rb[2 * a]); b[2 * a + 1] = fmaxf(lb[2 * a + 1], rb[2 * a + 1]); }
        for (int k = 0; k < 6; k++) o.box[6 * (size_t)node + k] = b[k];
        const int cnt = node_count(o, l) + node_count(o, r);
        o.count[node] = cnt;
        const bool collapse = refit(o, node, l, r, half_area(b), cnt);
        o.emitted[node] = collapse ? 0 : 1 + node_emitted(o, l) + node_emitted(o, r);
        node = o.parent[node];
    }
}

// d(n): inner nodes above n (the root's is 0), at the start of a pass.
__global__ __launch_bounds__(kBlock) void k_depth(Opt o) {
    if (!resolve(o)) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= o.m) return;
    int d = 0, c = i;
    for (int step = 0; step < kMaxClimb; step++) {
        const int a = o.parent[c];
        if (a < 0) break;
        d++;
        c = a;
    }
    o.depth[i] = d;
}

// Per-wave treelet state in LDS (1.2 KiB; a subset's area and triangle count stay in the registers of the lane that owns it).
struct TreeletLds {
    float box[kTreelet][6], slot_area[kTreelet], slot_cost[kTreelet];
    int id[kTreelet], cnt[kTreelet], hgt[kTreelet], expanded[kTreelet - 2];
    float cost[kSubsets];
    uint8_t part[kSubsets], height[kSubsets];
    int set[kTreelet - 1], node[kTreelet - 1], lc[kTreelet - 1], rc[kTreelet - 1];
    int stack[kTreelet + 1];                             // lane 0's pre-order walk (a private array would be promoted to 64 copies)
    int go;
};

__device__ __forceinline__ void load_slot(const Opt& o, TreeletLds& t, int k, int id) {
    t.id[k] = id;
    const float* b = node_box(o, id);
    for (int a = 0; a < 6; a++) t.box[k][a] = b[a];
    t.slot_area[k] = half_area(t.box[k]);
}

// One treelet, by the whole wave (all 64 lanes, wave-uniform control flow; the block is one wave, so __syncthreads orders LDS).
//   growth (lane 0): the slots start as the root's children; 5 times the slot of largest area among those holding an inner node
//     (ties: the lowest slot) is replaced by its left child, its right child goes to the next free slot
//   subsets (2 per lane): box union, area, triangle count of each of the 127 non-empty subsets of the 7 slots
//   DP by subset size 2 ... 7 (2 per lane): the best split of S into P and S ^ P, P over the submasks of S holding S's lowest slot
//     (S itself excluded) in increasing order, the first of least C(P) + C(S ^ P) wins; C(S) as in the rules above
//   accept (lane 0): the new topology's height must be at most kMaxDepth - d(root); otherwise the treelet stays as it is and
//     only the root's height and cost are refitted from its current children
//   rewrite (lanes 0 ... 5): the new inner nodes in pre-order (left part first) take the ids root, then the expanded nodes in
//     expansion order
__device__ void treelet(const Opt& o, int root, int* info, TreeletLds& t) {
    const int lane = threadIdx.x;
    if (lane == 0) {
        t.go = 1;
        const int l = o.left[root], r = o.right[root];
        if (valid_id(o, l) && valid_id(o, r)) { load_slot(o, t, 0, l); load_slot(o, t, 1, r); } else t.go = 0;
        for (int e = 0; e < kTreelet - 2 && t.go; e++) {
            const int k = 2 + e;
            int best = -1;
            for (int j = 0; j < k; j++)
                if (t.id[j] < o.m && (best < 0 || t.slot_area[j] > t.slot_area[best])) best = j;
            if (best < 0) { t.go = 0; break; }
            const int c = t.id[best], cl = o.left[c], cr = o.right[c];
            if (!valid_id(o, cl) || !valid_id(o, cr)) { t.go = 0; break; }
            t.expanded[e] = c;
            load_slot(o, t, best, cl);
            load_slot(o, t, k, cr);
        }
    }
    __syncthreads();
    if (!t.go) return;
    if (lane < kTreelet) {
        const int id = t.id[lane];
        t.cnt[lane] = node_count(o, id);
        t.slot_cost[lane] = node_cost(o, id);
        t.hgt[lane] = node_height(o, id);
    }
    __syncthreads();
    float area[2] = {0.0f, 0.0f};                        // subsets lane and lane + 64: the same lane does their DP below
    int tris[2] = {0, 0};
    for (int h = 0; h < 2; h++) {
        const int S = lane + 64 * h;
        if (S == 0) continue;
        float b[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
        int cnt = 0;
        for (int i = 0; i < kTreelet; i++)
            if ((S >> i) & 1) {
                for (int a = 0; a < 3; a++) { b[2 * a] = fminf(b[2 * a], t.box[i][2 * a]); b[2 * a + 1] = fmaxf(b[2 * a + 1], t.box[i][2 * a + 1]); }
                cnt += t.cnt[i];
            }
        area[h] = half_area(b);
        tris[h] = cnt;
        if (__popc(S) == 1) { const int i = __ffs(S) - 1; t.cost[S] = t.slot_cost[i]; t.height[S] = (uint8_t)t.hgt[i]; }
    }
    __syncthreads();
    for (int size = 2; size <= kTreelet; size++) {
        for (int h = 0; h < 2; h++) {
            const int S = lane + 64 * h;
            if (__popc(S) != size) continue;
            const int low = S & -S, rest = S ^ low;
            float best = 0.0f;
            int bp = -1, q = 0;
            do {                                         // the submasks of rest in increasing order
                if (q != rest) {
                    const int P = low | q;
                    const float c = t.cost[P] + t.cost[S ^ P];
                    if (bp < 0 || c < best) { best = c; bp = P; }
                }
                q = (q - rest) & rest;
            } while (q != 0);
            const float inner = o.node_cost * area[h] + best;
            float c = inner;
            if (tris[h] <= o.max_leaf) {
                const float leafc = (o.tri_cost * area[h]) * (float)tris[h];
                if (leafc <= inner) c = leafc;
            }
            t.cost[S] = c;
            t.part[S] = (uint8_t)bp;
        }
        __syncthreads();
    }
    if (lane == 0) {
        int sp = 0;
        t.stack[sp++] = kSubsets - 1;
        for (int j = 0; j < kTreelet - 1; j++) {
            const int S = t.stack[--sp], P = t.part[S], Q = S ^ P;
            t.set[j] = S;
            if (__popc(Q) >= 2) t.stack[sp++] = Q;
            if (__popc(P) >= 2) t.stack[sp++] = P;
        }
        for (int j = kTreelet - 2; j >= 0; j--) {
            const int S = t.set[j], P = t.part[S];
            t.height[S] = (uint8_t)(1 + max((int)t.height[P], (int)t.height[S ^ P]));
        }
        t.go = (int)t.height[kSubsets - 1] <= kMaxDepth - o.depth[root];
        if (!t.go) {
            // kept as it is: the root's height and cost still come from its children, which this pass may have restructured (its
            // ancestors read both, for their DP and for the depth rule); its box and count have not changed
            atomicAdd(&info[3], 1);
            refit(o, root, o.left[root], o.right[root], half_area(o.box + 6 * (size_t)root), o.count[root]);
        }
        for (int j = 0; j < kTreelet - 1; j++) t.node[j] = j == 0 ? root : t.expanded[j - 1];
        for (int j = 0; j < kTreelet - 1; j++) {
            const int S = t.set[j], part[2] = {t.part[S], S ^ t.part[S]};
            int ids[2];
            for (int k = 0; k < 2; k++) {
                const int X = part[k];
                if (__popc(X) == 1) {
                    ids[k] = t.id[__ffs(X) - 1];
                } else {
                    ids[k] = -1;
                    for (int i = 0; i < kTreelet - 1; i++) if (t.set[i] == X) ids[k] = t.node[i];
                }
            }
            t.lc[j] = ids[0]; t.rc[j] = ids[1];
        }
    }
    __syncthreads();
    if (t.go && lane < kTreelet - 1) {
        const int S = t.set[lane], node = t.node[lane], l = t.lc[lane], r = t.rc[lane];
        float b[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
        int cnt = 0;
        for (int i = 0; i < kTreelet; i++)
            if ((S >> i) & 1) {
                for (int a = 0; a < 3; a++) { b[2 * a] = fminf(b[2 * a], t.box[i][2 * a]); b[2 * a + 1] = fmaxf(b[2 * a + 1], t.box[i][2 * a + 1]); }
                cnt += t.cnt[i];
            }
        o.left[node] = l; o.right[node] = r;
        set_parent(o, l, node); set_parent(o, r, node);
        for (int k = 0; k < 6; k++) o.box[6 * (size_t)node + k] = b[k];
        o.count[node] = cnt;
        o.cost[node] = t.cost[S];
        o.height[node] = t.height[S];
    }
    __syncthreads();                                     // the LDS state is reused by the next treelet
}

// One treelet pass.  One thread per sorted triangle climbs as in k_bottom_up; per step the wave publishes what it wrote (agent
// release, then the wait, UNCONDITIONALLY, so that it drains the stores of every lane that took part in the last treelet), each
// climbing lane adds to its node's counter, the second arrivers acquire.  The lanes whose node holds at least gamma triangles are
// gathered by a ballot and the wave restructures their treelets one at a time, lowest lane first.  Arrival order decides only which
// wave handles a node: a node is reached once its two subtrees are final, and a treelet writes nodes of its own subtree only.
__global__ __launch_bounds__(64) void k_treelet(Opt o, int gamma, uint32_t* arrivals, int* info) {
    __shared__ TreeletLds t;
    if (!resolve(o)) return;                             // uniform over the block
    const int p = blockIdx.x * 64 + threadIdx.x;
    int node = p < o.n ? o.leaf_parent[p] : -1;
    bool active = node >= 0;
    for (int step = 0; step < kMaxClimb; step++) {
        if (__ballot(active) == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool own = false;
        if (active) own = __hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        active = own;
        uint64_t ready = __ballot(own && o.count[node] >= gamma);
        while (ready) {
            const int lane = __ffsll((unsigned long long)ready) - 1;
            ready &= ready - 1;
            treelet(o, __shfl(node, lane), info, t);
        }
        if (own) { node = o.parent[node]; active = node >= 0; }
    }
}

// Node2 records in depth-first pre-order: a node is emitted when it is inner, not collapsed and has no collapsed ancestor; its index
// and first triangle come from a walk to the root (a right child adds its left sibling's emitted count + 1 and triangle count).
__global__ __launch_bounds__(kBlock) void k_emit_opt_nodes(Opt o, Node2* __restrict__ nodes, int* info) {
    if (!resolve(o)) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= o.m) return;
    if (o.emitted[i] == 0) {
        if (i == 0) {                                   // the root collapsed: one root whose child 0 is the whole leaf
            Node2 nd;
            for (int k = 0; k < 6; k++) nd.bounds[k] = o.box[k];
            for (int a = 0; a < 3; a++) { nd.bounds[6 + 2 * a] = INFINITY; nd.bounds[7 + 2 * a] = -INFINITY; }
            nd.child[0] = ~0; nd.child[1] = 0; nd.pad[0] = nd.pad[1] = 0;
            nodes[0] = nd;
            info[kInfoNodes] = 1;
            atomicMax(&info[kInfoDepth], 1);
        }
        return;
    }
    int c = i, idx = 0, off = 0, level = 0;
    for (int step = 0; step < kMaxClimb; step++) {
        const int a = o.parent[c];
        if (a < 0) break;
        if (o.emitted[a] == 0) return;                  // inside a collapsed ancestor's leaf
        const int l = o.left[a];
        if (l != c) { idx += 1 + node_emitted(o, l); off += node_count(o, l); } else { idx += 1; }
        level++;
        c = a;
    }
    if (c != 0 || idx < 0 || idx >= o.m) return;         // not reached the root within the bound: a malformed tree, nothing written
    const int l = o.left[i], r = o.right[i];
    if (!valid_id(o, l) || !valid_id(o, r)) return;
    const float *lb = node_box(o, l), *rb = node_box(o, r);
    const int el = node_emitted(o, l);
    const int child0 = el > 0 ? idx + 2 : ~off;
    const int child1 = node_emitted(o, r) > 0 ? idx + 2 + el : ~(off + node_count(o, l));
    float4* out = reinterpret_cast<float4*>(nodes + idx);
    out[0] = make_float4(lb[0], lb[1], lb[2], lb[3]);
    out[1] = make_float4(lb[4], lb[5], rb[0], rb[1]);
    out[2] = make_float4(rb[2], rb[3], rb[4], rb[5]);
    out[3] = make_float4(__int_as_float(child0), __int_as_float(child1), 0.0f, 0.0f);
    atomicMax(&info[kInfoDepth], level + 1);
    if (i == 0) info[kInfoNodes] = o.emitted[0];
}

// Tri1 records in left-to-right leaf order; the end-of-leaf bit goes on the last triangle of the topmost collapsed node above the
// triangle (or of the triangle itself).
__global__ __launch_bounds__(kBlock) void k_emit_opt_tris(Opt o, const float4* __restrict__ vertices, int nv,
                                                          const int4* __restrict__ indices, const uint32_t* __restrict__ order,
                                                          Tri1* __restrict__ tris, const int* __restrict__ reftri) {
    if (!resolve(o)) return;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= o.n) return;
    int c = o.m + p, top = c, off = 0, within = 0;
    for (int step = 0; step < kMaxClimb; step++) {
        const int a = parent_of(o, c);
        if (a < 0) break;
        const int l = o.left[a];
        if (l != c) off += node_count(o, l);
        if (o.emitted[a] == 0) { top = a; within = off; }
        c = a;
    }
    if (c != 0 || off < 0 || off >= o.n) return;
    const bool last = within == node_count(o, top) - 1;
    const int t = reftri ? reftri[order[p]] : (int)order[p];
    float3 v[3]; int geom;
    load_triangle(vertices, nv, indices, t, v, &geom, nullptr);
    const TriGeometry g = tri1_geometry(v);
    float4* out = reinterpret_cast<float4*>(tris + off);
    out[0] = make_float4(g.v0.x, g.v0.y, g.v0.z, 0.0f);
    out[1] = make_float4(g.e1.x, g.e1.y, g.e1.z, __int_as_float(geom));
    out[2] = make_float4(g.e2.x, g.e2.y, g.e2.z, __int_as_float((int)((uint32_t)t | (last ? kLastInLeaf : 0u))));
}

// ---- 9. triangle pre-splitting (Karras & Aila 2013, section 5; the rules in include/rodent_build.h) -----------------------------
// Per triangle: k_split_boxes (box, frame partials, flags), k_split_frame, k_priority (p and its max), k_weights (w and W), k_allot
// (s and the block totals of s + 1), a scan, k_split (the pieces, in the triangle's slot range), a scan of the pieces made (n' in
// info[4]), k_refs (the references in order, their Morton points and point bounds).  Then launch_tree and the tails over n'.
constexpr int kSplitSteps = 4096;   // a cut loop takes at most 2 * 63 + 1 cuts and emits plus 3 * 1023 one-sided cuts (each removes a plane)
enum { kInfoRefs = 4, kInfoSplit = 5, kInfoUnmade = 6 };

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
    size_t off = 0;
    const auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return p; };
    const size_t N = (size_t)n, R = (size_t)max_refs, NB = (N + kBlock - 1) / kBlock;
    q.tbox = (float*)take(4 * 6 * N); q.prio = (float*)take(4 * N);
    q.w = (uint32_t*)take(4 * N); q.s = (uint32_t*)take(4 * N); q.start = (uint32_t*)take(4 * N); q.made = (uint32_t*)take(4 * N);
    q.blocktot = (uint32_t*)take(4 * NB); q.blockmade = (uint32_t*)take(4 * NB);
    q.kpartial = (float*)take(4 * 6 * NB);
    q.sframe = (float*)take(4 * 8);
    q.pmax = (uint32_t*)take(16); q.wsum = q.pmax ? (unsigned long long*)(q.pmax + 2) : nullptr;
    q.pbox = (float*)take(4 * 6 * R); q.pk = (int*)take(4 * R);
    q.refbox = (float*)take(4 * 6 * R); q.reftri = (int*)take(4 * R);
    q.bytes = off;
    return q;
}

// Block-wide min / max of per-thread bounds into out[6] (lo_x lo_y lo_z hi_x hi_y hi_z: the layout of k_centroids' partials).
__device__ void block_bounds(float lo[3], float hi[3], float* out) {
    __shared__ float red[6][kBlock];
    for (int a = 0; a < 3; a++) { red[a][threadIdx.x] = lo[a]; red[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 3; a++) {
                red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
                red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = red[threadIdx.x][0];
}

// Exclusive scan of v over the block (every thread takes part; once per kernel), the block's total in *total.
__device__ uint32_t block_scan(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wsum[kBlock / 64];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kBlock / 64; k++) { before += k < w ? wsum[k] : 0u; all += wsum[k]; }
    *total = all;
    return before + x - v;
}

// Canonical vertices of triangle t (x + 0: no -0), as rows V[vertex][axis]; returns the error flags.
__device__ __forceinline__ int load_canon(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int t,
                                          float V[3][3], int* info) {
    float3 v[3]; int geom;
    const int flags = load_triangle(vertices, nv, indices, t, v, &geom, info);
    for (int k = 0; k < 3; k++) { V[k][0] = canon(v[k].x); V[k][1] = canon(v[k].y); V[k][2] = canon(v[k].z); }
    return flags;
}

__global__ __launch_bounds__(kBlock) void k_split_boxes(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                        int n, float* __restrict__ tbox, float* __restrict__ partial, int* info) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        float V[3][3];
        load_canon(vertices, nv, indices, t, V, info);
        for (int a = 0; a < 3; a++) {
            const float l = fminf(fminf(V[0][a], V[1][a]), V[2][a]), h = fmaxf(fmaxf(V[0][a], V[1][a]), V[2][a]);
            tbox[6 * (size_t)t + 2 * a] = l; tbox[6 * (size_t)t + 2 * a + 1] = h;
            lo[a] = fminf(lo[a], l); hi[a] = fmaxf(hi[a], h);
        }
    }
    block_bounds(lo, hi, partial + 6 * blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_split_frame(const float* __restrict__ partial, int blocks, float* __restrict__ sframe) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < blocks; b += kBlock)
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partial[6 * b + a]); hi[a] = fmaxf(hi[a], partial[6 * b + 3 + a]); }
    __shared__ float out[6];
    block_bounds(lo, hi, out);
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float step = (out[3 + a] - out[a]) * 0x1p-10f;
        sframe[a] = out[a];
        sframe[3 + a] = (step > 0.0f && isfinite(step)) ? step : 0.0f;     // 0: the axis has no planes
    }
}

// The plane of box b: the coarsest grid plane strictly inside it, ties to x, y, z.  Returns its level (-1: none), *axis and *x.
// Per axis two binary searches over the monotone positions lo + (float)c * step give the planes strictly inside, c in [cmin, cmax];
// the coarsest of them keeps the bits above the highest bit where cmin - 1 and cmax differ.
__device__ __forceinline__ int find_plane(const float* __restrict__ sframe, const float b[6], int* axis, float* x) {
    int best = -1;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = sframe[a], step = sframe[3 + a];
        if (!(step > 0.0f)) continue;
        int c0 = 1, h0 = 1024, c1 = 1, h1 = 1024;        // first c with pos > b_lo, first c with pos >= b_hi (1024: none)
        for (int it = 0; it < 10; it++) {
            const int m0 = (c0 + h0) >> 1, m1 = (c1 + h1) >> 1;
            if (c0 < h0) { if (lo + (float)m0 * step > b[2 * a]) h0 = m0; else c0 = m0 + 1; }
            if (c1 < h1) { if (lo + (float)m1 * step >= b[2 * a + 1]) h1 = m1; else c1 = m1 + 1; }
        }
        const int cmin = c0, cmax = c1 - 1;
        if (cmin > cmax) continue;
        const int level = 31 - __clz((cmin - 1) ^ cmax), c = (cmax >> level) << level;
        if (level > best) { best = level; *axis = a; *x = lo + (float)c * step; }
    }
    return best;
}

__device__ __forceinline__ float pick(const float v[3], int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// The SBVH reference split of the triangle V's piece B at plane (axis, x) into boxes L and R (empty: lo > hi on some axis).  Fully
// unrolled, the axis selected by compares: no runtime-indexed private array.
__device__ __forceinline__ void cut(const float V[3][3], const float B[6], int axis, float x, float L[6], float R[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) { L[k] = (k & 1) ? -INFINITY : INFINITY; R[k] = L[k]; }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float* P = V[i];
        const float* Q = V[(i + 1) % 3];
        const float pa = pick(P, axis), qa = pick(Q, axis);
#pragma unroll
        for (int b = 0; b < 3; b++) {
            if (pa <= x) { L[2 * b] = fminf(L[2 * b], P[b]); L[2 * b + 1] = fmaxf(L[2 * b + 1], P[b]); }
            if (pa >= x) { R[2 * b] = fminf(R[2 * b], P[b]); R[2 * b + 1] = fmaxf(R[2 * b + 1], P[b]); }
        }
        if ((pa < x && qa > x) || (pa > x && qa < x)) {
            const float t = __fdiv_rn(x - pa, qa - pa);
#pragma unroll
            for (int b = 0; b < 3; b++) {
                float lo = x, hi = x;
                if (b != axis) {
                    const float y = P[b] + t * (Q[b] - P[b]);
                    const float g = fmaxf(fmaxf(fabsf(P[b]), fabsf(Q[b])) * 0x1p-19f, 0x1p-126f);
                    lo = fmaxf(y - g, fminf(P[b], Q[b]));
                    hi = fminf(y + g, fmaxf(P[b], Q[b]));
                }
                L[2 * b] = fminf(L[2 * b], lo); L[2 * b + 1] = fmaxf(L[2 * b + 1], hi);
                R[2 * b] = fminf(R[2 * b], lo); R[2 * b + 1] = fmaxf(R[2 * b + 1], hi);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 3; b++) {
        L[2 * b] = fmaxf(L[2 * b], B[2 * b]); L[2 * b + 1] = fminf(L[2 * b + 1], B[2 * b + 1]);
        R[2 * b] = fmaxf(R[2 * b], B[2 * b]); R[2 * b + 1] = fminf(R[2 * b + 1], B[2 * b + 1]);
        if (b == axis) { L[2 * b + 1] = fminf(L[2 * b + 1], x); R[2 * b] = fmaxf(R[2 * b], x); }
    }
}

__device__ __forceinline__ bool box_empty(const float b[6]) { return b[0] > b[1] || b[2] > b[3] || b[4] > b[5]; }
__device__ __forceinline__ float longest(const float b[6]) { return fmaxf(fmaxf(b[1] - b[0], b[3] - b[2]), b[5] - b[4]); }

__global__ __launch_bounds__(kBlock) void k_priority(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                     int n, const float* __restrict__ tbox, const float* __restrict__ sframe,
                                                     float* __restrict__ prio, uint32_t* pmax) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    float p = 0.0f;
    if (t < n) {
        float V[3][3];
        if (!load_canon(vertices, nv, indices, t, V, nullptr)) {
            float b[6];
            for (int k = 0; k < 6; k++) b[k] = tbox[6 * (size_t)t + k];
            int axis; float x;
            const int level = find_plane(sframe, b, &axis, &x);
            if (level >= 0) {
                const float ex = V[1][0] - V[0][0], ey = V[1][1] - V[0][1], ez = V[1][2] - V[0][2];
                const float fx = V[2][0] - V[0][0], fy = V[2][1] - V[0][1], fz = V[2][2] - V[0][2];
                const float nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
                const float excess = fmaxf(0.0f, half_area(b) - 0.5f * ((fabsf(nx) + fabsf(ny)) + fabsf(nz)));
                p = __fsqrt_rn((float)(1 << level) * excess);
                if (!isfinite(p)) p = 0.0f;
            }
        }
        prio[t] = p;
    }
    float m = p;
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (lane_id() == 0) atomicMax(pmax, __float_as_uint(m));
}

__global__ __launch_bounds__(kBlock) void k_weights(const float* __restrict__ prio, int n, const uint32_t* __restrict__ pmax,
                                                    uint32_t* __restrict__ w, unsigned long long* wsum) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const float top = __uint_as_float(*pmax);
    uint32_t wt = 0;
    if (t < n) {
        if (top > 0.0f) wt = (uint32_t)floorf(__fdiv_rn(prio[t], top) * 65536.0f);
        w[t] = wt;
    }
    uint32_t sum = wt;                                   // at most 64 * 65536 per wave
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane_id() == 0 && sum) atomicAdd(wsum, (unsigned long long)sum);
}

__global__ __launch_bounds__(kBlock) void k_allot(const uint32_t* __restrict__ w, int n, long long budget, int max_pieces,
                                                  const unsigned long long* __restrict__ wsum, uint32_t* __restrict__ s,
                                                  uint32_t* __restrict__ blocktot, int* info) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long W = *wsum;
    uint32_t st = 0;
    if (t < n) {
        if (W) st = (uint32_t)std::min((unsigned long long)(max_pieces - 1), ((unsigned long long)w[t] * (unsigned long long)budget) / W);
        s[t] = st;
    }
    const uint64_t split = __ballot(st > 0);
    if (lane_id() == 0 && split) atomicAdd(&info[kInfoSplit], (int)__popcll(split));
    uint32_t total;
    block_scan(t < n ? st + 1 : 0u, &total);
    if (threadIdx.x == 0) blocktot[blockIdx.x] = total;
}

// One thread per triangle cuts it into at most s + 1 pieces inside its slot range [start, start + s]: final pieces from the front,
// pending ones (box + splits) on a stack growing down from the back.  Every pending piece ends as at least one final piece and every
// cut spends a split, so (final pieces) + (pending pieces) <= s + 1: the two ends never meet.
__global__ __launch_bounds__(kBlock) void k_split(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int n,
                                                  const float* __restrict__ tbox, const float* __restrict__ sframe,
                                                  const uint32_t* __restrict__ s, const uint32_t* __restrict__ blockoff,
                                                  float* __restrict__ pbox, int* __restrict__ pk, uint32_t* __restrict__ start,
                                                  uint32_t* __restrict__ made, uint32_t* __restrict__ blockmade, int* info) {
    __shared__ uint32_t block_made;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int st = t < n ? (int)s[t] : 0;
    uint32_t total;
    const uint32_t first = blockoff[blockIdx.x] + block_scan(t < n ? (uint32_t)st + 1 : 0u, &total);
    if (threadIdx.x == 0) block_made = 0;
    __syncthreads();
    int out = 1;
    if (t < n && st > 0) {
        float V[3][3], cb[6];
        load_canon(vertices, nv, indices, t, V, nullptr);
        for (int k = 0; k < 6; k++) cb[k] = tbox[6 * (size_t)t + k];
        int k = st, sp = 0, unmade = 0;
        out = 0;
        for (int step = 0; step < kSplitSteps; step++) {
            int axis = 0; float x = 0.0f;
            bool final = k == 0 || find_plane(sframe, cb, &axis, &x) < 0;
            if (!final) {
                float L[6], R[6];
                cut(V, cb, axis, x, L, R);
                const bool le = box_empty(L), re = box_empty(R);
                if (le && re) {
                    final = true;
                } else if (le || re) {                   // the piece lies on one side: it takes that side's box and keeps its splits
                    for (int j = 0; j < 6; j++) cb[j] = le ? R[j] : L[j];
                    continue;
                } else {
                    const float el = longest(L), er = longest(R);
                    const float q = __fdiv_rn((float)(k - 1) * el, el + er);
                    const int kl = (int)fminf(fmaxf(floorf(q + 0.5f), 0.0f), (float)(k - 1));
                    const size_t slot = first + (size_t)(st - sp);
                    for (int j = 0; j < 6; j++) pbox[6 * slot + j] = R[j];
                    pk[slot] = k - 1 - kl;
                    sp++;
                    for (int j = 0; j < 6; j++) cb[j] = L[j];
                    k = kl;
                    continue;
                }
            }
            unmade += k;
            const size_t slot = first + (size_t)out;
            for (int j = 0; j < 6; j++) pbox[6 * slot + j] = canon(cb[j]);
            out++;
            if (sp == 0) break;
            sp--;
            const size_t top = first + (size_t)(st - sp);
            for (int j = 0; j < 6; j++) cb[j] = pbox[6 * top + j];
            k = pk[top];
        }
        if (unmade) atomicAdd(&info[kInfoUnmade], unmade);
    }
    if (t < n) { start[t] = first; made[t] = (uint32_t)out; atomicAdd(&block_made, (uint32_t)out); }
    __syncthreads();
    if (threadIdx.x == 0) blockmade[blockIdx.x] = block_made;
}

// References in order: per triangle its pieces (or, uncut, its box and vertex sum), their Morton points and the block's point bounds.
__global__ __launch_bounds__(kBlock) void k_refs(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int n,
                                                 const float* __restrict__ tbox, const uint32_t* __restrict__ s,
                                                 const uint32_t* __restrict__ start, const uint32_t* __restrict__ made,
                                                 const uint32_t* __restrict__ blockoff, const float* __restrict__ pbox,
                                                 float* __restrict__ refbox, int* __restrict__ reftri, float4* __restrict__ cent,
                                                 float* __restrict__ kpartial) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    const uint32_t dst = blockoff[blockIdx.x] + block_scan(t < n ? made[t] : 0u, &total);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (t < n) {
        if (s[t] == 0) {
            float3 v[3]; int geom;
            load_triangle(vertices, nv, indices, t, v, &geom, nullptr);
            const float c[3] = {(v[0].x + v[1].x) + v[2].x, (v[0].y + v[1].y) + v[2].y, (v[0].z + v[1].z) + v[2].z};
            for (int k = 0; k < 6; k++) refbox[6 * (size_t)dst + k] = tbox[6 * (size_t)t + k];
            reftri[dst] = t;
            cent[dst] = make_float4(c[0], c[1], c[2], 0.0f);
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
        } else {
            const uint32_t count = made[t];
            for (uint32_t j = 0; j < count; j++) {
                const float* b = pbox + 6 * ((size_t)start[t] + j);
                float c[3];
                for (int a = 0; a < 3; a++) c[a] = (b[2 * a] + b[2 * a + 1]) * 1.5f;
                for (int k = 0; k < 6; k++) refbox[6 * ((size_t)dst + j) + k] = b[k];
                reftri[dst + j] = t;
                cent[dst + j] = make_float4(c[0], c[1], c[2], 0.0f);
                for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
            }
        }
    }
    block_bounds(lo, hi, kpartial + 6 * blockIdx.x);
}

// ---- 11. refit: the boxes and Tri1 records of an existing hierarchy from moved vertices (rules: include/rodent_build.h) --------------
// The topology (child, pad and w words) is read and never written.  k_refit_links gives every inner child its parent slot, k_refit_tris
// rewrites the records and leaves their boxes in scratch, k_refit_climb fills the boxes bottom-up.  A node is complete after
// 1 + (children with id > 0) arrivals at its counter: its own thread's, once its leaf slots are filled, and one per inner child.  The
// last arriver unions the node's 12 bounds into its slot of the parent and arrives there; nobody waits for anybody, and since every
// value of a counter is returned once, a node is completed at most once: a malformed tree (a cycle, a child id out of range, a child
// claimed twice) leaves nodes incomplete, never a thread looping or a read out of bounds.
enum { kInfoRefitNodes = 0, kInfoRefitTris = 1 };

struct RefitScratch {
    int* parent;                  // per node: 2 * parent + slot, -1 = none (the root)
    uint32_t* arrivals;           // per node
    float* tribox;                // per Tri1 record: the box of its triangle
    size_t bytes;
};

RefitScratch carve_refit(char* base, int num_nodes, int num_bvh_tris) {
    RefitScratch s{};
    size_t off = 0;
    const auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return p; };
    s.parent = (int*)take(4 * (size_t)num_nodes);
    s.arrivals = (uint32_t*)take(4 * (size_t)num_nodes);
    s.tribox = (float*)take(4 * 6 * (size_t)num_bvh_tris);
    s.bytes = off;
    return s;
}

// Sum of `v` over the wave (every lane takes part), in every lane.
__device__ __forceinline__ int wave_sum(int v) {
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
    return v;
}

__global__ __launch_bounds__(kBlock) void k_refit_links(const Node2* __restrict__ nodes, int num_nodes, int num_bvh_tris, int* parent,
                                                        uint32_t* __restrict__ arrivals, int* info) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= num_nodes) return;
    arrivals[i] = 0u;
    int flags = 0;
    for (int k = 0; k < 2; k++) {
        const int c = nodes[i].child[k];
        if (c > 0) {
            // node 0 is the root: nobody's child.  A child that already has a parent slot keeps it.
            if (c > num_nodes || c == 1 || atomicCAS(&parent[c - 1], -1, 2 * i + k) != -1) flags |= RODENT_BUILD_BAD_TOPOLOGY;
        } else if (c < 0 && ~c >= num_bvh_tris) {
            flags |= RODENT_BUILD_BAD_TOPOLOGY;
        }
    }
    if (flags) atomicOr(&info[kInfoFlags], flags);
}

__global__ __launch_bounds__(kBlock) void k_refit_tris(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                       int num_tris, Tri1* __restrict__ tris, int num_bvh_tris,
                                                       float* __restrict__ tribox, int* info) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    bool done = false;
    if (p < num_bvh_tris) {
        float4* rec = reinterpret_cast<float4*>(tris + p);
        const float4 w2 = rec[2];
        const int t = (int)((uint32_t)__float_as_int(w2.w) & ~kLastInLeaf);
        float box[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
        if (t < num_tris) {
            float3 v[3]; int geom;
            load_triangle(vertices, nv, indices, t, v, &geom, info);
            const TriGeometry g = tri1_geometry(v);
            rec[0] = make_float4(g.v0.x, g.v0.y, g.v0.z, rec[0].w);
            rec[1] = make_float4(g.e1.x, g.e1.y, g.e1.z, rec[1].w);
            rec[2] = make_float4(g.e2.x, g.e2.y, g.e2.z, w2.w);
            triangle_box(v, box);
            done = true;
        } else {
            atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);      // the record stays as it is, its box is empty
        }
        for (int k = 0; k < 6; k++) tribox[6 * (size_t)p + k] = box[k];
    }
    const int count = __syncthreads_count(done);
    if (threadIdx.x == 0 && count) atomicAdd(&info[kInfoRefitTris], count);
}

__global__ __launch_bounds__(kBlock) void k_refit_climb(Node2* nodes, int num_nodes, const Tri1* __restrict__ tris, int num_bvh_tris,
                                                        const float* __restrict__ tribox, const int* __restrict__ parent,
                                                        uint32_t* arrivals, int* info) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int node = i < num_nodes ? i : -1;
    if (node >= 0) {
        for (int k = 0; k < 2; k++) {
            const int c = nodes[node].child[k];
            if (c >= 0 || ~c >= num_bvh_tris) continue;          // empty, inner, or flagged by k_refit_links: the slot stays as stored
            float b[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
            bool ended = false;
            for (int p = ~c; p < num_bvh_tris && !ended; p++) {
                const float* tb = tribox + 6 * (size_t)p;
                for (int a = 0; a < 3; a++) { b[2 * a] = fminf(b[2 * a], tb[2 * a]); b[2 * a + 1] = fmaxf(b[2 * a + 1], tb[2 * a + 1]); }
                ended = tris[p].prim_id < 0;
            }
            if (ended) for (int j = 0; j < 6; j++) nodes[node].bounds[6 * k + j] = b[j];
            else atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);       // a leaf without an end bit
        }
    }
    bool active = node >= 0;
    int completed = 0;
    // wave-uniform: the release and its wait cover the stores of every lane before any lane of the wave adds
    for (int step = 0; step <= num_nodes; step++) {
        if (__ballot(active) == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool last = false;
        if (active) {
            const uint32_t needed = 1u + (nodes[node].child[0] > 0) + (nodes[node].child[1] > 0);
            last = __hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == needed - 1u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        active = false;
        if (last) {
            completed++;
            const int up = parent[node];
            if (up >= 0) {
                const float* b = nodes[node].bounds;
                float u[6];
                for (int a = 0; a < 3; a++) { u[2 * a] = fminf(b[2 * a], b[6 + 2 * a]); u[2 * a + 1] = fmaxf(b[2 * a + 1], b[7 + 2 * a]); }
                node = up >> 1;
                for (int j = 0; j < 6; j++) nodes[node].bounds[6 * (up & 1) + j] = u[j];
                active = true;
            }
        }
    }
    completed = wave_sum(completed);
    if (lane_id() == 0 && completed) atomicAdd(&info[kInfoRefitNodes], completed);
}

inline int blocks_for(long long items) { return (int)((items + kBlock - 1) / kBlock); }

bool set_device(int32_t dev) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && dev >= 0 && dev < count && hipSetDevice(dev) == hipSuccess;
}

int32_t check_args(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris, int32_t max_leaf,
                   const void* nodes, const void* tris, const void* scratch, const int32_t* info_dev) {
    if (num_tris < 1 || num_tris > kMaxTris) return RODENT_BUILD_ERR_NUM_TRIS;
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

// Morton codes (from s.cent and s.frame), the sort, the sorted leaves and (n > 1) the Karras hierarchy.  With `nref` (split) the
// grids are sized for n = max_refs and every kernel runs over the n' = *nref references (reftri / refbox: their triangles and boxes).
void launch_tree(const Scratch& s, const float4* v4, int nv, const int4* i4, int n, int max_leaf, Tri1* tris, const int* nref,
                 const int* reftri, const float* refbox, hipStream_t stream) {
    const int m = n - 1;
    hipLaunchKernelGGL(k_morton, dim3(blocks_for(n)), dim3(kBlock), 0, stream, s.cent, n, s.frame, s.keys[0], s.vals[0], nref);
    const int tiles = radix_tiles(n);
    for (int pass = 0; pass < 4; pass++) {                       // 30 key bits: 8 + 8 + 8 + 6; four passes end in buffer 0
        const int in = pass & 1, shift = 8 * pass;
        hipLaunchKernelGGL(k_radix_hist, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], n, shift, s.hist, nref);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.hist, 256 * tiles, (int*)nullptr);
        hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], s.vals[in], s.keys[in ^ 1],
                           s.vals[in ^ 1], s.hist, n, shift, nref);
    }
    hipLaunchKernelGGL(k_leaves, dim3(blocks_for(n)), dim3(kBlock), 0, stream, v4, nv, i4, s.vals[0], n, tris, s.leafbox, nref,
                       reftri, refbox);
    if (m > 0)
        hipLaunchKernelGGL(k_karras, dim3(blocks_for(m)), dim3(kBlock), 0, stream, s.keys[0], n, max_leaf, s.first, s.last, s.split,
                           s.parent, s.leaf_parent, s.blockcount, nref);
}

// The LBVH tail: renumbering, boxes and heights, Node2 records.  Without `nref` the host knows n and launches either k_emit or the
// single-leaf root; with it both are launched and each writes only when n' calls for it.
void launch_lbvh_tail(const Scratch& s, int n, int max_leaf, Node2* nodes, Tri1* tris, int32_t* info_dev, const int* nref,
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
        hipLaunchKernelGGL(k_emit, dim3(blocks_for(m)), dim3(kBlock), 0, stream, m, s.first, s.last, s.split, s.newidx, s.leafbox,
                           s.box, nodes, tris, nref);
    if (nref || n <= max_leaf)
        hipLaunchKernelGGL(k_emit_root, dim3(1), dim3(1), 0, stream, n, s.leafbox, s.box, nodes, tris, info_dev, nref, max_leaf);
}

// The optimising tail: the explicit tree, k_fit, the treelet passes, k_fit again, pre-order emission.  Without `nref` it is only
// reached with n > 1; with it the single-leaf root follows, written when n' = 1.  False when a memset is refused.
bool launch_opt_tail(const Scratch& s, int n, const RodentBuildOptions& opt, const float4* v4, int nv, const int4* i4, Node2* nodes,
                     Tri1* tris, int32_t* info_dev, const int* nref, const int* reftri, hipStream_t stream) {
    const int m = n - 1;
    if (m > 0) {
        Opt o{};
        o.n = n; o.m = m; o.max_leaf = opt.max_leaf; o.node_cost = opt.node_cost; o.tri_cost = opt.tri_cost;
        o.left = s.left; o.right = s.right; o.parent = s.parent; o.leaf_parent = s.leaf_parent; o.count = s.count; o.height = s.height;
        o.emitted = s.emitted; o.depth = s.depth; o.box = s.box; o.cost = s.cost; o.leafbox = s.leafbox; o.nref = nref;
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
    if (nref) hipLaunchKernelGGL(k_emit_root, dim3(1), dim3(1), 0, stream, n, s.leafbox, s.box, nodes, tris, info_dev, nref, 1);
    return true;
}

// Every entry after its argument checks: info words and arrival counters zeroed, the front (centroids, or with `split` the
// pre-splitting stages of section 9), launch_tree, then the LBVH tail (treelet_passes = 0) or the optimising one.  Without `split`
// the stages run over the n triangles; with it over the n' references, on grids sized for max_refs.
int32_t launch_build(const float* vertices, int nv, const int32_t* indices, int n, const RodentBuildOptions& opt,
                     const RodentSplitOptions* split, Node2* nodes, Tri1* tris, void* scratch, int32_t* info_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int R = split ? (int)split_max_refs(n, split) : n, M = R - 1;
    const bool optimise = opt.treelet_passes > 0;
    const Scratch s = carve(static_cast<char*>(scratch), R, optimise);
    const SplitScratch q = split ? carve_split(static_cast<char*>(scratch) + s.bytes, n, R) : SplitScratch{};
    const float4* v4 = reinterpret_cast<const float4*>(vertices);
    const int4* i4 = reinterpret_cast<const int4*>(indices);
    const int* nref = split ? info_dev + kInfoRefs : nullptr;     // n', written by the second scan; every later stage reads it
    // an unsplit caller's info buffer may hold only RODENT_BUILD_INFO_WORDS words
    const size_t info_bytes = 4 * (size_t)(split ? RODENT_BUILD_SPLIT_INFO_WORDS : RODENT_BUILD_INFO_WORDS);
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
    launch_tree(s, v4, nv, i4, R, opt.max_leaf, tris, nref, q.reftri, q.refbox, stream);
    if (!optimise)
        launch_lbvh_tail(s, R, opt.max_leaf, nodes, tris, info_dev, nref, stream);
    else if (!launch_opt_tail(s, R, opt, v4, nv, i4, nodes, tris, info_dev, nref, q.reftri, stream))
        return RODENT_BUILD_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

// The refit after its argument checks: info words zeroed, parent slots set to -1, then the three kernels of section 11.
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

} // namespace

extern "C" {

int64_t rodent_hip_build_scratch_bytes(int32_t num_tris) {
    if (num_tris < 1 || num_tris > kMaxTris) return -1;
    return (int64_t)carve(nullptr, num_tris).bytes;
}

int32_t rodent_hip_build_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev,
                                   void* stream) {
    const int32_t rc = check_args(dev, vertices, num_vertices, indices, num_tris, max_leaf, nodes, tris, scratch, info_dev);
    if (rc != RODENT_BUILD_OK) return rc;
    const RodentBuildOptions opt{max_leaf, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    return launch_build(vertices, num_vertices, indices, num_tris, opt, nullptr, nodes, tris, scratch, info_dev, stream);
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
    if (num_tris < 1 || num_tris > kMaxTris || check_options(opt) != RODENT_BUILD_OK) return -1;
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
    return launch_build(vertices, num_vertices, indices, num_tris, o, nullptr, nodes, tris, scratch, info_dev, stream);
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
    if (num_tris < 1 || num_tris > kMaxTris || check_split(split) != RODENT_BUILD_OK) return -1;
    return split_max_refs(num_tris, split);
}

int64_t rodent_hip_build_split_scratch_bytes(int32_t num_tris, const struct RodentBuildOptions* opt,
                                             const struct RodentSplitOptions* split) {
    if (num_tris < 1 || num_tris > kMaxTris || check_options(opt) != RODENT_BUILD_OK || check_split(split) != RODENT_BUILD_OK) return -1;
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
    return launch_build(vertices, num_vertices, indices, num_tris, *opt, split, nodes, tris, scratch, info_dev, stream);
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

int64_t rodent_hip_refit_scratch_bytes(int32_t num_nodes, int32_t num_bvh_tris) {
    if (num_nodes < 1 || num_bvh_tris < 1) return -1;
    return (int64_t)carve_refit(nullptr, num_nodes, num_bvh_tris).bytes;
}

int32_t rodent_hip_refit_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   struct Node2* nodes, int32_t num_nodes, struct Tri1* tris, int32_t num_bvh_tris, void* scratch,
                                   int32_t* info_dev, void* stream) {
    if (num_tris < 1 || num_tris > kMaxTris) return RODENT_BUILD_ERR_NUM_TRIS;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (num_nodes < 1 || num_bvh_tris < 1) return RODENT_BUILD_ERR_NUM_NODES;
    if (!vertices || !indices || !nodes || !tris || !scratch || !info_dev) return RODENT_BUILD_ERR_NULL;
    if (!set_device(dev)) return RODENT_BUILD_ERR_DEVICE;
    return launch_refit(vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, scratch, info_dev, stream);
}

int32_t rodent_hip_refit_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, struct Node2* nodes, int32_t num_nodes, struct Tri1* tris,
                                        int32_t num_bvh_tris, int32_t* info) {
    const int64_t bytes = rodent_hip_refit_scratch_bytes(num_nodes, num_bvh_tris);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_NODES;
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    int32_t rc = build_sync(dev, bytes, RODENT_BUILD_INFO_WORDS, words, [&](void* scratch, int32_t* info_dev) {
        return rodent_hip_refit_bvh2_tri1(dev, vertices, num_vertices, indices, num_tris, nodes, num_nodes, tris, num_bvh_tris, scratch,
                                          info_dev, nullptr);
    });
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    if (rc == RODENT_BUILD_OK && words[kInfoRefitNodes] != num_nodes) rc = RODENT_BUILD_ERR_INPUT;    // a malformed topology
    return rc;
}

} // extern "C"
