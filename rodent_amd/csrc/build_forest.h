// build_forest.h -- the forest form of the LBVH builder (included by bvh_build.hip after build_refit.h): the hierarchies of a list of
// objects built in ONE launch list, straight into the packed arrays of an instanced scene (rodent_hip_build_objects,
// include/rodent_instances.h; CPU model: tests/forest_build_model.py).
#pragma once
// The stages of build_lbvh.h over the listed objects' triangles laid end to end, the arrangement of k_forest_* (build_refit.h): position
// p of the triangle space belongs to the range r with ranges[r].rec_start <= p < ranges[r + 1].rec_start, found by bisection
// (forest_range<true>), and everything a stage keeps of an object lies in the object's own stretch of the scratch arrays, at rec_start,
// with object-local values: Karras node i of an object at rec_start + i (one slot per object stays unused).  Unsorted position
// rec_start + t is row t of the object; the sort is by (range, code, row), so an object's sorted triangles fill its stretch again.
// What a range claims is checked before anything of it is indexed (build_span): a range that fails has nothing touched.  Scratch values
// that a faulty range table could leave stale (overlapping stretches) are checked before they index anything, and every climb is
// bounded by the object's triangle count.
struct BuildForest {
    RodentObject* objects; const RodentRefitRange* ranges;
    int num_objects, num_listed, total_tris, num_rows, max_leaf, pack;
    int* object_info;                                    // 4 words per listed object: Node2 count, depth, flags, 0
    int* info;                                           // the call's: total nodes, largest depth, OR of the flags, 0
    uint32_t* fbounds;                                   // 6 per listed object: the ordered bits of its centroid-sum bounds (lo, then hi)
    uint32_t* objnodes;                                  // per listed object: its Node2 count, scanned in place to its packed node offset
};

struct BuildSpan {
    int rank;                                            // its place in the list
    int node_offset, tri_offset;                         // where its records go (in place: the table's; pack: tri_offset = rec_start,
                                                         // node_offset from objnodes once that is scanned: build_node_offset)
    int object, first_tri, n, start;                     // its table entry, its rows of the index table, its stretch [start, start + n)
    int flags;                                           // 0: sound
};

__device__ __forceinline__ BuildSpan build_span(const BuildForest& a, int r) {
    const RodentRefitRange g = a.ranges[r];
    BuildSpan s{};
    s.rank = r; s.object = g.object; s.first_tri = g.first_tri; s.n = g.num_tris; s.start = g.rec_start; s.tri_offset = g.rec_start;
    if ((unsigned)g.object >= (unsigned)a.num_objects) { s.flags = RODENT_TLAS_BAD_OBJECT; return s; }
    bool sound = g.first_tri >= 0 && g.num_tris >= 1 && g.first_tri <= a.num_rows - g.num_tris && g.node_start == g.rec_start
        && g.rec_start >= 0 && g.rec_start <= a.total_tris - g.num_tris;
    if (!a.pack) {
        const RodentObject o = a.objects[g.object];
        s.node_offset = o.node_offset; s.tri_offset = o.tri_offset;
        sound = sound && o.num_tris == g.num_tris && o.node_offset >= 0 && o.tri_offset >= 0;
    }
    if (!sound) s.flags = RODENT_BUILD_BAD_TOPOLOGY;
    return s;
}

__device__ __forceinline__ ForestArgs build_ranges(const BuildForest& a) {
    return ForestArgs{a.objects, a.ranges, a.num_objects, a.num_listed, 0, a.total_tris, a.num_rows};
}

// The span of position p and p's place in it; false when p lies in no sound range (a refused one, or a gap of a faulty table).
__device__ __forceinline__ bool build_at(const BuildForest& a, int p, BuildSpan* s, int* local) {
    *s = build_span(a, forest_range<true>(build_ranges(a), p));
    *local = p - s->start;
    return !s->flags && *local >= 0 && *local < s->n;
}

// The most Node2 records of an object of n triangles, and the node offset of a span once objnodes is scanned.
__device__ __forceinline__ int build_node_room(int n) { return max(1, n - 1); }
__device__ __forceinline__ int build_node_offset(const BuildForest& a, const BuildSpan& s) {
    return a.pack ? (int)a.objnodes[s.rank] : s.node_offset;
}

// Floats as unsigned integers in the same order (no NaN comes here): min / max by integer atomics, exact in any order.
__device__ __forceinline__ uint32_t ordered_bits(float x) {
    const uint32_t b = (uint32_t)__float_as_int(x);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float ordered_float(uint32_t u) { return __int_as_float((int)(u & 0x80000000u ? u & 0x7FFFFFFFu : ~u)); }

__device__ __forceinline__ void build_flag(const BuildForest& a, int rank, int flags) {
    atomicOr(&a.object_info[4 * rank + kInfoFlags], flags);
    atomicOr(&a.info[kInfoFlags], flags);
}

// ---- 0. one thread per listed object: the range's own flag, its info words, empty bounds --------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bf_begin(BuildForest a) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.num_listed) return;
    const int flags = build_span(a, j).flags;
    a.object_info[4 * j] = 0; a.object_info[4 * j + 1] = 0; a.object_info[4 * j + 2] = flags; a.object_info[4 * j + 3] = 0;
    if (flags) atomicOr(&a.info[kInfoFlags], flags);
    a.objnodes[j] = 0u;
    for (int k = 0; k < 3; k++) { a.fbounds[6 * j + k] = ordered_bits(INFINITY); a.fbounds[6 * j + 3 + k] = ordered_bits(-INFINITY); }
}

// ---- 1. centroid sums and each object's bounds of them ---------------------------------------------------------------------------------
// k_centroids per position.  A block whose positions lie in one range reduces its bounds (block_reduce) and six threads add them to the
// object's; a block across ranges adds per thread.  fminf / fmaxf skip a NaN, so a NaN is never added.
__global__ __launch_bounds__(kBlock) void k_bf_centroids(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                         BuildForest a, float4* __restrict__ cent) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    BuildSpan s{}; int t = 0;
    const bool mine = p < a.total_tris && build_at(a, p, &s, &t);
    if (mine) {
        float3 v[3]; int geom;
        const int flags = load_triangle(vertices, nv, indices + s.first_tri, t, v, &geom, a.object_info + 4 * s.rank);
        if (flags) atomicOr(&a.info[kInfoFlags], flags);
        const float c[3] = {(v[0].x + v[1].x) + v[2].x, (v[0].y + v[1].y) + v[2].y, (v[0].z + v[1].z) + v[2].z};
        cent[p] = make_float4(c[0], c[1], c[2], 0.0f);
        for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], c[k]); hi[k] = fmaxf(hi[k], c[k]); }
    }
    // the same for every thread of the block: its first and its last position find one range
    const int head = blockIdx.x * kBlock, tail = min(head + kBlock, a.total_tris) - 1;
    const int r0 = forest_range<true>(build_ranges(a), head);
    if (r0 == forest_range<true>(build_ranges(a), tail)) {
        const float (*red)[kBlock] = block_reduce(lo, hi);
        if (threadIdx.x < 6) {
            const float b = red[threadIdx.x][0];
            if (threadIdx.x < 3 && b < INFINITY) atomicMin(&a.fbounds[6 * r0 + threadIdx.x], ordered_bits(b));
            if (threadIdx.x >= 3 && b > -INFINITY) atomicMax(&a.fbounds[6 * r0 + threadIdx.x], ordered_bits(b));
        }
    } else if (mine) {
        for (int k = 0; k < 3; k++) {
            if (lo[k] < INFINITY) atomicMin(&a.fbounds[6 * s.rank + k], ordered_bits(lo[k]));
            if (hi[k] > -INFINITY) atomicMax(&a.fbounds[6 * s.rank + 3 + k], ordered_bits(hi[k]));
        }
    }
}

// ---- 2. Morton codes in the object's own frame -----------------------------------------------------------------------------------------
// k_bounds' frame rule and k_morton's cell per position.  A position in no sound range gets the largest key: it sorts behind its
// range's triangles and nothing reads it.  code0 keeps the unsorted codes (the sort's buffers are overwritten): k_bf_leaves gathers them.
__global__ __launch_bounds__(kBlock) void k_bf_morton(BuildForest a, const float4* __restrict__ cent, uint32_t* __restrict__ code0,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.total_tris) return;
    BuildSpan s; int t;
    uint32_t code = 0xFFFFFFFFu;
    if (build_at(a, p, &s, &t)) {
        const float4 c = cent[p];
        const float q3[3] = {c.x, c.y, c.z};
        uint32_t cell[3];
        for (int k = 0; k < 3; k++) {
            const float l = ordered_float(a.fbounds[6 * s.rank + k]), extent = ordered_float(a.fbounds[6 * s.rank + 3 + k]) - l;
            // an axis without extent (or with a non-finite one) gets cell 0 everywhere, never a division by zero
            const float scale = (extent > 0.0f && isfinite(extent)) ? __fdiv_rn(1024.0f, extent) : 0.0f;
            const float q = (q3[k] - l) * scale;
            cell[k] = (uint32_t)fminf(fmaxf(q, 0.0f), 1023.0f);     // fmaxf takes 0 over a NaN
        }
        code = (spread10(cell[0]) << 2) | (spread10(cell[1]) << 1) | spread10(cell[2]);
    }
    code0[p] = code; keys[p] = code; vals[p] = (uint32_t)p;
}

// The keys of the rank passes: the range of every sorted value (its unsorted position).
__global__ __launch_bounds__(kBlock) void k_bf_rank_keys(BuildForest a, const uint32_t* __restrict__ vals, uint32_t* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.total_tris) return;
    const uint32_t p = vals[i];
    keys[i] = p < (uint32_t)a.total_tris ? (uint32_t)forest_range<true>(build_ranges(a), (int)p) : 0u;
}

// ---- 4. leaves: Tri1 records where they stay, boxes and codes in sorted order ----------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bf_leaves(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                      BuildForest a, const uint32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ code0, Tri1* __restrict__ tris,
                                                      float* __restrict__ leafbox, uint32_t* __restrict__ codes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.total_tris) return;
    BuildSpan s; int local;
    if (!build_at(a, i, &s, &local)) return;
    const uint32_t p = order[i];
    const int t = (int)p - s.start;
    if (p >= (uint32_t)a.total_tris || t < 0 || t >= s.n) {          // a faulty range table: the sort left another range's position here
        build_flag(a, s.rank, RODENT_BUILD_BAD_TOPOLOGY);
        codes[i] = 0u;
        for (int k = 0; k < 6; k++) leafbox[6 * (size_t)i + k] = k & 1 ? -INFINITY : INFINITY;
        return;
    }
    float3 v[3]; int geom;
    load_triangle(vertices, nv, indices + s.first_tri, t, v, &geom, nullptr);
    store_tri1(tris + s.tri_offset + local, tri1_geometry(v), geom, t);
    triangle_box(v, leafbox + 6 * (size_t)i);
    codes[i] = code0[p];
}

// ---- 5. Karras hierarchy, every position object-local ----------------------------------------------------------------------------------
// k_karras with `codes`, the node arrays and the positions i, j relative to the object's stretch: delta() sees the object's n codes
// alone, so j outside [0, n) gives -1, ties fall back to the local positions, and no search leaves the object.
__global__ __launch_bounds__(kBlock) void k_bf_karras(BuildForest a, const uint32_t* __restrict__ allcodes, int* __restrict__ first,
                                                      int* __restrict__ last, int* __restrict__ split, int* __restrict__ parent,
                                                      int* __restrict__ leaf_parent, uint32_t* __restrict__ blockcount) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false;
    BuildSpan s{}; int i = 0;
    if (p < a.total_tris && build_at(a, p, &s, &i) && i < s.n - 1) {
        const uint32_t* codes = allcodes + s.start;
        const int n = s.n;
        const int d = delta(codes, n, i, i + 1) > delta(codes, n, i, i - 1) ? 1 : -1;
        const int dmin = delta(codes, n, i, i - d);
        int lmax = 2;
        while (delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
        int l = 0;
        for (int t = lmax >> 1; t >= 1; t >>= 1)
            if (delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
        const int j = i + l * d, dnode = delta(codes, n, i, j);
        int sp = 0, t = l;
        do {
            t = (t + 1) >> 1;
            if (delta(codes, n, i, i + (sp + t) * d) > dnode) sp += t;
        } while (t > 1);
        const int g = i + sp * d + min(d, 0), f = min(i, j), e = max(i, j);
        first[s.start + i] = f; last[s.start + i] = e; split[s.start + i] = g;
        if (f == g) leaf_parent[s.start + g] = i; else parent[s.start + g] = i;
        if (e == g + 1) leaf_parent[s.start + g + 1] = i; else parent[s.start + g + 1] = i;
        if (i == 0) parent[s.start] = -1;
        kept = e - f + 1 > a.max_leaf;
    }
    const int count = __syncthreads_count(kept);
    if (threadIdx.x == 0) blockcount[blockIdx.x] = (uint32_t)count;
}

// A Karras node's stored range, checked: only a faulty range table leaves anything else in the object's stretch.
__device__ __forceinline__ bool build_node(const BuildSpan& s, const int* first, const int* last, const int* split, int node, int* f,
                                           int* e, int* g) {
    *f = first[s.start + node]; *e = last[s.start + node]; *g = split[s.start + node];
    return *f >= 0 && *f <= *g && *g < *e && *e < s.n;
}

// ---- the kept nodes' ranks: k_renumber over all positions, the exclusive scan value of EVERY position (kept or not) --------------------
// A kept node's new index is gidx[its position] - gidx[its object's first position]; an object's Node2 count the difference over its
// whole stretch (its last, unused slot is never kept).
__global__ __launch_bounds__(kBlock) void k_bf_renumber(BuildForest a, const int* __restrict__ first, const int* __restrict__ last,
                                                        const uint32_t* __restrict__ blockoff, uint32_t* __restrict__ gidx) {
    __shared__ uint32_t wave_total[kBlock / 64];
    const int p = blockIdx.x * kBlock + threadIdx.x, w = threadIdx.x >> 6;
    BuildSpan s{}; int i = 0;
    const bool kept = p < a.total_tris && build_at(a, p, &s, &i) && i < s.n - 1 && last[p] - first[p] + 1 > a.max_leaf;
    const uint64_t b = __ballot(kept);
    if (lane_id() == 0) wave_total[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t idx = blockoff[blockIdx.x] + (uint32_t)__popcll(b & lanes_below());
    for (int k = 0; k < w; k++) idx += wave_total[k];
    if (p < a.total_tris) gidx[p] = idx;
}

// The new index of local node `node` of span s, or -1 when it is not kept (e - f + 1 <= max_leaf) or the index leaves the object's room.
__device__ __forceinline__ int build_newidx(const BuildForest& a, const BuildSpan& s, const uint32_t* __restrict__ gidx, int node, int f,
                                            int e) {
    if (e - f + 1 <= a.max_leaf) return -1;
    const uint32_t idx = gidx[s.start + node] - gidx[s.start];
    return idx < (uint32_t)build_node_room(s.n) ? (int)idx : -1;
}

// One thread per listed object: its Node2 count, for the scan that gives the packed node offsets and the total.
__global__ __launch_bounds__(kBlock) void k_bf_counts(BuildForest a, const uint32_t* __restrict__ gidx) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.num_listed) return;
    const BuildSpan s = build_span(a, j);
    if (s.flags) return;                                 // objnodes[j] = 0 (k_bf_begin)
    const uint32_t kept = gidx[s.start + s.n - 1] - gidx[s.start];
    const int count = s.n <= a.max_leaf ? 1 : (int)min(max(kept, 1u), (uint32_t)build_node_room(s.n));
    a.objnodes[j] = (uint32_t)count;
    a.object_info[4 * j + kInfoNodes] = count;
}

// ---- 6. bottom-up boxes and heights: k_bottom_up's hand-off, ending at the object's local node 0 ---------------------------------
__global__ __launch_bounds__(kBlock) void k_bf_bottom_up(BuildForest a, const int* __restrict__ first, const int* __restrict__ last,
                                                         const int* __restrict__ split, const int* __restrict__ parent,
                                                         const int* __restrict__ leaf_parent, const float* __restrict__ leafbox,
                                                         float* box, int* height, uint32_t* arrivals) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    BuildSpan s; int local;
    if (p >= a.total_tris || !build_at(a, p, &s, &local) || s.n < 2) return;
    const float* const lbox = leafbox + 6 * (size_t)s.start;
    float* const nbox = box + 6 * (size_t)s.start;
    int* const h_of = height + s.start;
    int node = leaf_parent[p];
    for (int step = 0; step < s.n && node >= 0; step++) {        // a climb visits fewer than n nodes
        if (node >= s.n - 1) { build_flag(a, s.rank, RODENT_BUILD_BAD_TOPOLOGY); return; }
        publish();
        if (arrive(&arrivals[s.start + node]) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        int f, e, g;
        if (!build_node(s, first, last, split, node, &f, &e, &g)) { build_flag(a, s.rank, RODENT_BUILD_BAD_TOPOLOGY); return; }
        const float* lb = f == g ? lbox + 6 * (size_t)g : nbox + 6 * (size_t)g;
        const float* rb = e == g + 1 ? lbox + 6 * (size_t)(g + 1) : nbox + 6 * (size_t)(g + 1);
        const int hl = f == g ? 0 : h_of[g], hr = e == g + 1 ? 0 : h_of[g + 1];
        unite(nbox + 6 * (size_t)node, lb, rb);
        const int h = e - f + 1 > a.max_leaf ? 1 + max(hl, hr) : 0;
        h_of[node] = h;
        if (node == 0 && h > 0) { a.object_info[4 * s.rank + kInfoDepth] = h; atomicMax(&a.info[kInfoDepth], h); }
        node = parent[s.start + node];
    }
}

// ---- 7. emission: k_emit's record to nodes + node_offset + newidx, end-of-leaf bits at tris + tri_offset -----------------------
__global__ __launch_bounds__(kBlock) void k_bf_emit(BuildForest a, const int* __restrict__ first, const int* __restrict__ last,
                                                    const int* __restrict__ split, const uint32_t* __restrict__ gidx,
                                                    const float* __restrict__ leafbox, const float* __restrict__ box,
                                                    Node2* __restrict__ nodes, Tri1* __restrict__ tris) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    BuildSpan s; int i;
    if (p >= a.total_tris || !build_at(a, p, &s, &i) || i >= s.n - 1 || s.n <= a.max_leaf) return;
    int f, e, g;
    if (!build_node(s, first, last, split, i, &f, &e, &g)) { build_flag(a, s.rank, RODENT_BUILD_BAD_TOPOLOGY); return; }
    const int mine = build_newidx(a, s, gidx, i, f, e);
    if (mine < 0) return;
    const float* const lbox = leafbox + 6 * (size_t)s.start;
    const float* const nbox = box + 6 * (size_t)s.start;
    Tri1* const recs = tris + s.tri_offset;
    const int lo[2] = {f, g + 1}, hi[2] = {g, e};                    // the children's sorted ranges
    float b[12];
    int child[2];
    for (int k = 0; k < 2; k++) {
        const int c = g + k;
        const bool single = lo[k] == hi[k];
        put_bounds(b + 6 * k, single ? lbox + 6 * (size_t)c : nbox + 6 * (size_t)c);
        int cf, ce, cg, cidx = -1;
        if (!single && c < s.n - 1 && build_node(s, first, last, split, c, &cf, &ce, &cg)) cidx = build_newidx(a, s, gidx, c, cf, ce);
        if (cidx >= 0) {
            child[k] = cidx + 1;
        } else {
            child[k] = ~lo[k];
            mark_last_in_leaf(recs + hi[k]);
        }
    }
    float4* out = reinterpret_cast<float4*>(nodes + build_node_offset(a, s) + mine);
    out[0] = make_float4(b[0], b[1], b[2], b[3]);
    out[1] = make_float4(b[4], b[5], b[6], b[7]);
    out[2] = make_float4(b[8], b[9], b[10], b[11]);
    out[3] = make_float4(__int_as_float(child[0]), __int_as_float(child[1]), 0.0f, 0.0f);
}

// One thread per listed object: the single-leaf root of an object of at most max_leaf triangles (k_emit_root), and the object's table
// entry: the whole RodentObject in pack mode, num_nodes alone in place.
__global__ __launch_bounds__(kBlock) void k_bf_objects(BuildForest a, const float* __restrict__ leafbox, const float* __restrict__ box,
                                                       Node2* __restrict__ nodes, Tri1* __restrict__ tris) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.num_listed) return;
    const BuildSpan s = build_span(a, j);
    if (s.flags) return;
    const int node_offset = build_node_offset(a, s);
    if (s.n <= a.max_leaf) {
        store_leaf_root(nodes + node_offset, (s.n == 1 ? leafbox : box) + 6 * (size_t)s.start);
        mark_last_in_leaf(tris + s.tri_offset + (s.n - 1));
        a.object_info[4 * j + kInfoDepth] = 1;
        atomicMax(&a.info[kInfoDepth], 1);
    }
    const int count = a.object_info[4 * j + kInfoNodes];
    if (a.pack) a.objects[s.object] = RodentObject{node_offset, s.tri_offset, count, s.n};
    else a.objects[s.object].num_nodes = count;
}
