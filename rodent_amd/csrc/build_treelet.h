// build_treelet.h -- stage 8 of the device BVH builder (included by bvh_build.hip after build_lbvh.h).
#pragma once
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
        publish();
        if (arrive(&arrivals[node]) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int l = o.left[node], r = o.right[node];
        if (!valid_id(o, l) || !valid_id(o, r)) return;
        const float *lb = node_box(o, l), *rb = node_box(o, r);
        float b[6];
        unite(b, lb, rb);
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
            if ((S >> i) & 1) { unite(b, b, t.box[i]); cnt += t.cnt[i]; }
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
            if ((S >> i) & 1) { unite(b, b, t.box[i]); cnt += t.cnt[i]; }
        o.left[node] = l; o.right[node] = r;
        set_parent(o, l, node); set_parent(o, r, node);
        for (int k = 0; k < 6; k++) o.box[6 * (size_t)node + k] = b[k];
        o.count[node] = cnt;
        o.cost[node] = t.cost[S];
        o.height[node] = t.height[S];
    }
    __syncthreads();                                     // the LDS state is reused by the next treelet
}

// One treelet pass.  One thread per sorted triangle climbs as in k_bottom_up, in the wave-uniform form of the hand-off (build_device.h):
// per step every lane publishes, each climbing lane arrives at its node's counter, the second arrivers acquire.  The lanes whose node holds
// at least gamma triangles are gathered by a ballot and the wave restructures their treelets one at a time, lowest lane first.  Arrival
// order decides only which wave handles a node: a node is reached once its two subtrees are final, and a treelet writes nodes of its own
// subtree only.
__global__ __launch_bounds__(64) void k_treelet(Opt o, int gamma, uint32_t* arrivals, int* info) {
    __shared__ TreeletLds t;
    if (!resolve(o)) return;                             // uniform over the block
    const int p = blockIdx.x * 64 + threadIdx.x;
    int node = p < o.n ? o.leaf_parent[p] : -1;
    bool active = node >= 0;
    for (int step = 0; step < kMaxClimb; step++) {
        if (__ballot(active) == 0) break;
        publish();
        bool own = false;
        if (active) own = arrive(&arrivals[node]) != 0u;
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
        if (i == 0) {                                   // the root collapsed: the single-leaf root
            store_leaf_root(nodes, o.box);
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
    store_tri1(tris + off, tri1_geometry(v), geom, (int)((uint32_t)t | (last ? kLastInLeaf : 0u)));
}
