// build_lbvh.h -- stages 1 to 7 of the device BVH builder, the LBVH (included by bvh_build.hip after build_device.h).
#pragma once
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
    block_bounds(lo, hi, partial + 6 * blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_bounds(const float* __restrict__ partial, int blocks, float* __restrict__ frame) {
    const float (*red)[kBlock] = reduce_partials(partial, blocks);
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
    store_tri1(tris + p, tri1_geometry(v), geom, t);
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
// One thread per sorted triangle climbs from its leaf.  At each node the hand-off of build_device.h: publish what this thread wrote and
// arrive at the node's counter; the first arriver stops, the second acquires and reads both children, one of them the other thread's.
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
        publish();
        if (arrive(&arrivals[node]) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int f = first[node], e = last[node], g = split[node];
        const float* lb = f == g ? leafbox + 6 * (size_t)g : box + 6 * (size_t)g;
        const float* rb = e == g + 1 ? leafbox + 6 * (size_t)(g + 1) : box + 6 * (size_t)(g + 1);
        const int hl = f == g ? 0 : height[g], hr = e == g + 1 ? 0 : height[g + 1];
        unite(box + 6 * (size_t)node, lb, rb);
        const int h = e - f + 1 > max_leaf ? 1 + max(hl, hr) : 0;
        height[node] = h;
        if (node == 0 && h > 0) info[kInfoDepth] = h;
        node = parent[node];
    }
}

// ---- 7. emission ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_bounds(float* dst, const float* b) { for (int k = 0; k < 6; k++) dst[k] = b[k]; }

// Rec: the leaf records, Tri1 or (build_tlas.h) RodentInstance; only their end-of-leaf bits are written here.
template <class Rec>
__global__ __launch_bounds__(kBlock) void k_emit(int m, const int* __restrict__ first, const int* __restrict__ last,
                                                 const int* __restrict__ split, const int* __restrict__ newidx,
                                                 const float* __restrict__ leafbox, const float* __restrict__ box,
                                                 Node2* __restrict__ nodes, Rec* __restrict__ tris, const int* nref) {
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
            mark_last_in_leaf(tris + hi[k]);
        }
    }
    float4* out = reinterpret_cast<float4*>(nodes + newidx[i]);
    out[0] = make_float4(b[0], b[1], b[2], b[3]);
    out[1] = make_float4(b[4], b[5], b[6], b[7]);
    out[2] = make_float4(b[8], b[9], b[10], b[11]);
    out[3] = make_float4(__int_as_float(child[0]), __int_as_float(child[1]), 0.0f, 0.0f);
}

// n <= max_leaf: the single-leaf root.  With `nref` (the split entry: n' on the device) it writes only when n' <= limit.
template <class Rec>
__global__ void k_emit_root(int n, const float* __restrict__ leafbox, const float* __restrict__ box, Node2* __restrict__ nodes,
                            Rec* __restrict__ tris, int* info, const int* nref, int limit) {
    if (nref) { n = *nref; if (n > limit) return; }
    store_leaf_root(nodes, n == 1 ? leafbox : box);
    mark_last_in_leaf(tris + (n - 1));
    info[kInfoNodes] = 1;
    info[kInfoDepth] = 1;
}
