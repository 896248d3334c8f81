// bvh_build.hip -- linear BVH builder on the device (LBVH: Morton codes + Karras 2012 hierarchy) writing BVH2 / Tri1 in the layout
// of include/rodent_traversal.h.  C ABI: include/rodent_build.h.  CPU model of every stage, byte for byte: tests/lbvh_model.py.
//
// Stages, all on the caller's stream, nothing allocated, no host synchronisation:
//   k_centroids      per triangle: indices checked before any vertex load, centroid sum s = (v0 + v1) + v2, per-block min / max
//   k_bounds         one block: the centroid bounds and per-axis scale = 1024 / extent (0 for an empty or non-finite extent)
//   k_morton         30-bit Morton code: cell = (uint)min(max((s - lo) * scale, 0), 1023) per axis, x in the highest bit of a triple
//   k_radix_*        stable LSD radix sort of (code, triangle id), 4 passes of 8 bits: order = by code, then by triangle id
//   k_leaves         Tri1 records in sorted order + the sorted triangles' boxes
//   k_karras         the n - 1 internal nodes (Karras 2012, delta ties broken by the sorted position), parent links, kept-node counts
//   k_renumber       kept internal nodes (more than max_leaf triangles) numbered by an exclusive scan in Karras order
//   k_bottom_up      boxes and heights, per-node arrival counters (first arriver leaves, the second goes on; no waiting)
//   k_emit / k_emit_root   Node2 records, end-of-leaf bits
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
    size_t bytes;
};

inline int radix_tiles(int n) { return (n + kRadixTile - 1) / kRadixTile; }

Scratch carve(char* base, int n) {
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
__device__ __forceinline__ void load_triangle(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int t,
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
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
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
__global__ __launch_bounds__(kBlock) void k_radix_hist(const uint32_t* __restrict__ keys, int n, int shift, uint32_t* __restrict__ hist) {
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
                                                          const uint32_t* __restrict__ hist, int n, int shift) {
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
                                                   float* __restrict__ leafbox) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int t = (int)order[p];
    float3 v[3]; int geom;
    load_triangle(vertices, nv, indices, t, v, &geom, nullptr);
    float4* out = reinterpret_cast<float4*>(tris + p);
    out[0] = make_float4(v[0].x, v[0].y, v[0].z, 0.0f);
    out[1] = make_float4(v[0].x - v[1].x, v[0].y - v[1].y, v[0].z - v[1].z, __int_as_float(geom));
    out[2] = make_float4(v[2].x - v[0].x, v[2].y - v[0].y, v[2].z - v[0].z, __int_as_float(t));
    const float c[3][3] = {{v[0].x, v[1].x, v[2].x}, {v[0].y, v[1].y, v[2].y}, {v[0].z, v[1].z, v[2].z}};
    for (int a = 0; a < 3; a++) {
        leafbox[6 * (size_t)p + 2 * a] = fminf(fminf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
        leafbox[6 * (size_t)p + 2 * a + 1] = fmaxf(fmaxf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
    }
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
                                                   int* __restrict__ leaf_parent, uint32_t* __restrict__ blockcount) {
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
                                                     const uint32_t* __restrict__ blockoff, int* __restrict__ newidx) {
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
                                                      float* box, int* height, uint32_t* arrivals, int* info) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
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
                                                 Node2* __restrict__ nodes, Tri1* __restrict__ tris) {
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

// n <= max_leaf: one root whose child 0 is the whole leaf; the empty slot as the host writer leaves it (+inf, -inf)
__global__ void k_emit_root(int n, const float* __restrict__ leafbox, const float* __restrict__ box, Node2* __restrict__ nodes,
                            Tri1* __restrict__ tris, int* info) {
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

inline int blocks_for(long long items) { return (int)((items + kBlock - 1) / kBlock); }

} // namespace

extern "C" {

int64_t rodent_hip_build_scratch_bytes(int32_t num_tris) {
    if (num_tris < 1 || num_tris > kMaxTris) return -1;
    return (int64_t)carve(nullptr, num_tris).bytes;
}

int32_t rodent_hip_build_bvh2_tri1(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_tris,
                                   int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, void* scratch, int32_t* info_dev,
                                   void* stream_) {
    if (num_tris < 1 || num_tris > kMaxTris) return RODENT_BUILD_ERR_NUM_TRIS;
    if (max_leaf < 1 || max_leaf > 8) return RODENT_BUILD_ERR_MAX_LEAF;
    if (num_vertices < 1) return RODENT_BUILD_ERR_NUM_VERTICES;
    if (!vertices || !indices || !nodes || !tris || !scratch || !info_dev) return RODENT_BUILD_ERR_NULL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count) return RODENT_BUILD_ERR_DEVICE;
    if (hipSetDevice(dev) != hipSuccess) return RODENT_BUILD_ERR_DEVICE;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int n = num_tris, m = n - 1;
    const Scratch s = carve(static_cast<char*>(scratch), n);
    const float4* v4 = reinterpret_cast<const float4*>(vertices);
    const int4* i4 = reinterpret_cast<const int4*>(indices);

    if (hipMemsetAsync(info_dev, 0, 4 * RODENT_BUILD_INFO_WORDS, stream) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    if (m > 0 && hipMemsetAsync(s.arrivals, 0, 4 * (size_t)m, stream) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    const int cblocks = std::min(kBoundsBlocks, blocks_for(n));
    hipLaunchKernelGGL(k_centroids, dim3(cblocks), dim3(kBlock), 0, stream, v4, num_vertices, i4, n, s.cent, s.partial, info_dev);
    hipLaunchKernelGGL(k_bounds, dim3(1), dim3(kBlock), 0, stream, s.partial, cblocks, s.frame);
    hipLaunchKernelGGL(k_morton, dim3(blocks_for(n)), dim3(kBlock), 0, stream, s.cent, n, s.frame, s.keys[0], s.vals[0]);
    const int tiles = radix_tiles(n);
    for (int pass = 0; pass < 4; pass++) {                       // 30 key bits: 8 + 8 + 8 + 6; four passes end in buffer 0
        const int in = pass & 1, shift = 8 * pass;
        hipLaunchKernelGGL(k_radix_hist, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], n, shift, s.hist);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.hist, 256 * tiles, (int*)nullptr);
        hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kBlock), 0, stream, s.keys[in], s.vals[in], s.keys[in ^ 1],
                           s.vals[in ^ 1], s.hist, n, shift);
    }
    hipLaunchKernelGGL(k_leaves, dim3(blocks_for(n)), dim3(kBlock), 0, stream, v4, num_vertices, i4, s.vals[0], n, tris, s.leafbox);
    if (m > 0) {
        const int kblocks = blocks_for(m);
        hipLaunchKernelGGL(k_karras, dim3(kblocks), dim3(kBlock), 0, stream, s.keys[0], n, max_leaf, s.first, s.last, s.split,
                           s.parent, s.leaf_parent, s.blockcount);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, stream, s.blockcount, kblocks, info_dev + kInfoNodes);
        hipLaunchKernelGGL(k_renumber, dim3(kblocks), dim3(kBlock), 0, stream, s.first, s.last, m, max_leaf, s.blockcount, s.newidx);
        hipLaunchKernelGGL(k_bottom_up, dim3(blocks_for(n)), dim3(kBlock), 0, stream, n, max_leaf, s.first, s.last, s.split, s.parent,
                           s.leaf_parent, s.leafbox, s.box, s.height, s.arrivals, info_dev);
    }
    if (n > max_leaf)
        hipLaunchKernelGGL(k_emit, dim3(blocks_for(m)), dim3(kBlock), 0, stream, m, s.first, s.last, s.split, s.newidx, s.leafbox,
                           s.box, nodes, tris);
    else
        hipLaunchKernelGGL(k_emit_root, dim3(1), dim3(1), 0, stream, n, s.leafbox, s.box, nodes, tris, info_dev);
    return hipGetLastError() == hipSuccess ? RODENT_BUILD_OK : RODENT_BUILD_ERR_LAUNCH;
}

int32_t rodent_hip_build_bvh2_tri1_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices,
                                        int32_t num_tris, int32_t max_leaf, struct Node2* nodes, struct Tri1* tris, int32_t* info) {
    const int64_t bytes = rodent_hip_build_scratch_bytes(num_tris);
    if (bytes < 0) return RODENT_BUILD_ERR_NUM_TRIS;
    if (max_leaf < 1 || max_leaf > 8) return RODENT_BUILD_ERR_MAX_LEAF;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count || hipSetDevice(dev) != hipSuccess)
        return RODENT_BUILD_ERR_DEVICE;
    void* scratch = nullptr;
    if (hipMalloc(&scratch, (size_t)bytes + 4 * RODENT_BUILD_INFO_WORDS) != hipSuccess) return RODENT_BUILD_ERR_LAUNCH;
    int32_t* info_dev = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + bytes);
    int32_t rc = rodent_hip_build_bvh2_tri1(dev, vertices, num_vertices, indices, num_tris, max_leaf, nodes, tris, scratch, info_dev,
                                            nullptr);
    int32_t words[RODENT_BUILD_INFO_WORDS] = {0, 0, 0, 0};
    if (rc == RODENT_BUILD_OK && hipMemcpy(words, info_dev, sizeof words, hipMemcpyDeviceToHost) != hipSuccess)
        rc = RODENT_BUILD_ERR_LAUNCH;
    (void)hipFree(scratch);
    if (info) for (int k = 0; k < RODENT_BUILD_INFO_WORDS; k++) info[k] = words[k];
    if (rc == RODENT_BUILD_OK && words[kInfoFlags]) rc = RODENT_BUILD_ERR_INPUT;
    return rc;
}

} // extern "C"
