// build_device.h -- what the stages of the device BVH builder share: constants, wave and block helpers, the arrival hand-off, triangle
// loads, boxes, the Tri1 and single-leaf-root stores.  Included first by bvh_build.hip, like the other build_*.h inside its namespace.
#pragma once
constexpr int kBlock = 256;
constexpr int kRadixItems = 16;                          // keys per thread and pass: a tile of 4096
constexpr int kRadixTile = kBlock * kRadixItems;
constexpr int kBoundsBlocks = 1024;                      // partial centroid bounds (grid-stride)
constexpr int kMaxTris = 1 << 25;
constexpr uint32_t kLastInLeaf = 0x80000000u;

enum { kInfoNodes = 0, kInfoDepth = 1, kInfoFlags = 2 };

// ---- wave64 helpers ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ uint64_t lanes_below() { return __lanemask_lt(); }

// Block-wide min / max of per-thread bounds: row k of the returned LDS array starts with the result (lo_x lo_y lo_z hi_x hi_y hi_z),
// readable by every thread on return.  Once per kernel: a second call would overwrite the rows the first one returned.
__device__ const float (*block_reduce(const float lo[3], const float hi[3]))[kBlock] {
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
    return red;
}
// ... into out[6], the layout of k_centroids' partials.
__device__ void block_bounds(const float lo[3], const float hi[3], float* out) {
    const float (*red)[kBlock] = block_reduce(lo, hi);
    if (threadIdx.x < 6) out[threadIdx.x] = red[threadIdx.x][0];
}
// ... over `blocks` partial bounds of that layout, by ONE block.
__device__ const float (*reduce_partials(const float* __restrict__ partial, int blocks))[kBlock] {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < blocks; b += kBlock)
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], partial[6 * b + a]); hi[a] = fmaxf(hi[a], partial[6 * b + 3 + a]); }
    return block_reduce(lo, hi);
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

// ---- the arrival hand-off of the bottom-up climbs (k_bottom_up, k_fit, k_treelet, k_refit_climb) --------------------------------------
// A thread that has written a node's inputs publishes them (agent-scope release, then its wait) and arrives at the node's counter (a
// relaxed agent-scope add returning the arrivals before it); whoever finds the counter complete acquires at agent scope (the caller's
// fence) and reads them all, some written on another XCD.  Nobody waits for anybody.  The wave-uniform climbs (k_treelet, k_refit_climb)
// publish in EVERY lane, UNCONDITIONALLY, on each step and arrive under `if (active)`: the release then drains the stores of every lane
// before any lane of the wave adds -- in k_treelet those of every lane that took part in the last treelet.
__device__ __forceinline__ void publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ uint32_t arrive(uint32_t* counter) {
    return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- boxes (lo_x hi_x lo_y hi_y lo_z hi_z) and triangles ------------------------------------------------------------------------------
// dst = the union of boxes a and b (dst may be a or b).
__device__ __forceinline__ void unite(float* dst, const float* a, const float* b) {
    for (int k = 0; k < 3; k++) { dst[2 * k] = fminf(a[2 * k], b[2 * k]); dst[2 * k + 1] = fmaxf(a[2 * k + 1], b[2 * k + 1]); }
}

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

// A Tri1 record: the geometry, the geometry id and the prim word (triangle id, bit 31: the last of its leaf); the first pad word is 0.
__device__ __forceinline__ void store_tri1(Tri1* rec, const TriGeometry& g, int geom, int prim) {
    float4* out = reinterpret_cast<float4*>(rec);
    out[0] = make_float4(g.v0.x, g.v0.y, g.v0.z, 0.0f);
    out[1] = make_float4(g.e1.x, g.e1.y, g.e1.z, __int_as_float(geom));
    out[2] = make_float4(g.e2.x, g.e2.y, g.e2.z, __int_as_float(prim));
}

// The end-of-leaf bit of a leaf record: bit 31 of a Tri1's prim_id, of a Rodent(Motion)Instance's instance_id (k_emit, k_emit_root).
__device__ __forceinline__ void mark_last_in_leaf(Tri1* rec) { rec->prim_id = (int32_t)((uint32_t)rec->prim_id | kLastInLeaf); }
__device__ __forceinline__ void mark_last_in_leaf(RodentInstance* rec) {
    rec->instance_id = (int32_t)((uint32_t)rec->instance_id | kLastInLeaf);
}
__device__ __forceinline__ void mark_last_in_leaf(RodentMotionInstance* rec) {
    rec->instance_id = (int32_t)((uint32_t)rec->instance_id | kLastInLeaf);
}

// The single-leaf root over box b: child 0 is the whole leaf, the empty second slot as the host writer leaves it (+inf, -inf).
__device__ __forceinline__ void store_leaf_root(Node2* nodes, const float* b) {
    Node2 nd;
    for (int k = 0; k < 6; k++) nd.bounds[k] = b[k];
    for (int a = 0; a < 3; a++) { nd.bounds[6 + 2 * a] = INFINITY; nd.bounds[7 + 2 * a] = -INFINITY; }
    nd.child[0] = ~0; nd.child[1] = 0; nd.pad[0] = nd.pad[1] = 0;
    nodes[0] = nd;
}

// The box of a triangle's corners taken as x + 0: lo_x hi_x lo_y hi_y lo_z hi_z.
__device__ __forceinline__ void triangle_box(const float3 v[3], float* box) {
    const float c[3][3] = {{v[0].x, v[1].x, v[2].x}, {v[0].y, v[1].y, v[2].y}, {v[0].z, v[1].z, v[2].z}};
    for (int a = 0; a < 3; a++) {
        box[2 * a] = fminf(fminf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
        box[2 * a + 1] = fmaxf(fmaxf(canon(c[a][0]), canon(c[a][1])), canon(c[a][2]));
    }
}
