// build_collapse.h -- BVH2 / Tri1 collapsed into Node4 / Node8 + Tri4 (included by bvh_build.hip after build_refit.h).
#pragma once
// ---- collapse (rules: include/rodent_build.h, "collapse into the wide layouts"; CPU model: tests/collapse_model.py) ----------------
// Every output word is a bit copy or an exact function of the Node2 and Tri1 records; no vertices.  Nobody waits for anybody: every
// thread derives what it needs by bounded walks of its own, there are no arrival counters, and the launches do not depend on the tree.
//   k_refit_links      (build_refit.h) parent slots, child ids and leaf starts checked
//   k_collapse_small   per node: the records of its subtree when it is small (at most 4, one behind the other), else 0
//   k_collapse_height  only with a stack limit: per inner node that is not small, H = the inner nodes that are not small on the longest
//                      path below it, itself included: each thread climbs its parent links and raises the heights with atomicMax
//   k_collapse_flags   per node: the climb to the root (at most 64 parents, the turns kept in a 64-bit word), then down again through the
//                      wide roots above it, simulating each one's expansion with "which slot is on my path": is this node a wide root?
//                      A wide root expands itself too and raises the stack bound B (atomicMax).  Leaf slots and topmost small nodes
//                      mark their packets per record.  With a stack limit every growth takes its root's S, the sum of
//                      (filled slots - 1) over the wide nodes above it, and a wide root's S is kept for k_collapse_nodes.
//   k_collapse_totals, k_scan, k_collapse_ids   twice: wide ids from the root flags, packet ids from the record marks
//   k_collapse_packets per marked record: its Tri4
//   k_collapse_nodes   per wide root: the expansion again, keeping per slot its source (node, side); the 6 bounds are copied at the end
// The N slots live in registers: every access is an unrolled compare-and-select, never a runtime index.
// Limited = false is the collapse without a stack limit: it reads no height and no S, and keeps no h in its slots.
enum { kInfoWideNodes = 0, kInfoPackets = 1, kInfoStackBound = 3 };
constexpr int kMaxRun = 64;                              // records of the longest run
// a record's mark: lanes of the packet that starts here (0: none starts), its last-in-leaf bit, "a leaf holds this record"
constexpr int kMarkLanes = 7, kMarkLast = 8, kMarkHeld = 16;

struct Collapse {
    const Node2* nodes; int num_nodes;
    const Tri1* tris; int num_bvh_tris;
    int* parent;                  // per node: 2 * parent + side, -1 = none (k_refit_links)
    int *small, *small_first;     // per node: records of a small subtree (0: not small) and the first of them
    int* root;                    // per node: 1 = a wide root
    int* mark;                    // per record (zeroed for every call)
    uint32_t *wide_id, *packet_id;    // exclusive scans of the root flags / of the records where a packet starts
    int* info;
    int *height, *above;          // with a stack limit only, per node: H (0: small) / the S a wide root is entered with
    int limit;                    // the stack limit L, 0 = none
};

__device__ __forceinline__ bool ends_leaf(const Collapse& c, int p) { return c.tris[p].prim_id < 0; }

// The records under inner node i when its subtree is small, else 0: the walk stops at the 5th record or the 4th inner node, so a
// cycle ends it too.  Three pending right children at most: a stack of three registers.
__device__ int small_records(const Collapse& c, int i, int* first_out) {
    int s0 = 0, s1 = 0, s2 = 0, pending = 0;
    int ref = i + 1, inner = 0, count = 0, next = -1, first = 0;
    for (int step = 0; step < 16; step++) {
        if (ref > 0) {
            if (ref > c.num_nodes || ++inner > 3) return 0;
            const int c0 = c.nodes[ref - 1].child[0], c1 = c.nodes[ref - 1].child[1];
            if (c0 != 0 && c1 != 0) { s2 = s1; s1 = s0; s0 = c1; pending++; }
            ref = c0 != 0 ? c0 : c1;
            if (ref != 0) continue;
        } else {
            const int s = ~ref;
            if (s >= c.num_bvh_tris || (next >= 0 && s != next)) return 0;
            if (next < 0) first = s;
            int p = s;
            bool ended = false;
            while (!ended) {
                if (p >= c.num_bvh_tris || ++count > 4) return 0;
                ended = ends_leaf(c, p++);
            }
            next = p;
        }
        if (pending == 0) { *first_out = first; return count; }
        ref = s0; s0 = s1; s1 = s2; pending--;
    }
    return 0;
}

__global__ __launch_bounds__(kBlock) void k_collapse_small(Collapse c) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_nodes) return;
    int first = 0;
    c.small[i] = small_records(c, i, &first);
    c.small_first[i] = first;
    if (c.limit > 0) c.height[i] = 0;
}

// H of every inner node that is not small (a small node keeps 0): 1 above the larger H of its children.  Thread i brings 1 to node i,
// 2 to its parent, 3 to the parent's parent ... and stops where the value already there is not smaller: the thread that put it there is
// carrying it on upward itself, so the array ends as the exact maximum whatever the order of the threads.  Nobody waits.  The parents
// of a node that is not small are not small either.
__global__ __launch_bounds__(kBlock) void k_collapse_height(Collapse c) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_nodes || c.small[i] != 0) return;
    int at = i;
    for (int h = 1; h <= kMaxClimb + 1; h++) {                    // the node and at most 64 parents
        if (atomicMax(&c.height[at], h) >= h) break;
        const int up = c.parent[at];
        if (up < 0) break;
        at = up >> 1;
    }
}

// `lanes` records from `first` become one packet, the last of its leaf when `last`.  A record two leaves hold raises the flag.
__device__ __forceinline__ int mark_packet(const Collapse& c, int first, int lanes, bool last) {
    int flags = 0;
    for (int k = 0; k < lanes; k++) {
        const int m = k ? kMarkHeld : kMarkHeld | lanes | (last ? kMarkLast : 0);
        if (atomicExch(&c.mark[first + k], m) != 0) flags = RODENT_BUILD_BAD_TOPOLOGY;
    }
    return flags;
}

// The packets of the plain run that starts at record s: ceil(k / 4) of them.  Returns the flags its guards raise.
__device__ int mark_run(const Collapse& c, int s) {
    if (s >= c.num_bvh_tris) return 0;                                               // flagged by k_refit_links
    if (s > 0 && !ends_leaf(c, s - 1)) return RODENT_BUILD_BAD_TOPOLOGY;              // a start inside another run
    int len = 0;
    bool ended = false;
    while (!ended) {
        if (s + len >= c.num_bvh_tris || len == kMaxRun) return RODENT_BUILD_BAD_TOPOLOGY;   // no end bit / a run too long
        ended = ends_leaf(c, s + len++);
    }
    int flags = 0;
    for (int q = 0; q < len; q += 4) flags |= mark_packet(c, s + q, min(4, len - q), q + 4 >= len);
    return flags;
}

// The slots of a wide node while it grows.  area: A of the slot's stored bounds when it can be expanded (a sound inner node that is
// not small), NaN otherwise: a NaN never wins.  h (with a stack limit): H of that inner node, 0 otherwise.
template <int N> struct Slots {
    int ref[N], src[N];           // the child reference and where its bounds are stored: 2 * node + side
    float area[N];
    int h[N];
    int count;
};

template <int N, bool Limited>
__device__ __forceinline__ void set_slot(const Collapse& c, Slots<N>& s, int j, int node, int side) {
    const Node2& nd = c.nodes[node];
    const int ref = nd.child[side];
    const bool open = ref > 1 && ref <= c.num_nodes && c.small[ref - 1] == 0;
    const float a = open ? half_area(nd.bounds + 6 * side) : __int_as_float(0x7FC00000);
    const int h = Limited && open ? c.height[ref - 1] : 0;
#pragma unroll
    for (int q = 0; q < N; q++)
        if (q == j) { s.ref[q] = ref; s.src[q] = 2 * node + side; s.area[q] = a; s.h[q] = h; }
}

// The slots a wide node rooted at r starts with: r's children that are not 0, in order.
template <int N, bool Limited> __device__ __forceinline__ void first_slots(const Collapse& c, Slots<N>& s, int r) {
#pragma unroll
    for (int q = 0; q < N; q++) { s.ref[q] = 0; s.src[q] = 0; s.area[q] = __int_as_float(0x7FC00000); s.h[q] = 0; }
    s.count = 0;
    for (int k = 0; k < 2; k++)
        if (c.nodes[r].child[k] != 0) set_slot<N, Limited>(c, s, s.count++, r, k);
}

// The slot to expand next: the largest A, the first of equals; -1 when none can be.  With a stack limit, in a node entered with S,
// slot j is a candidate only when S + count + h(s) <= limit for every other filled slot s: the largest h and the second largest
// (the largest of the others, for the slot that holds the largest) are found first.
template <int N, bool Limited> __device__ __forceinline__ int widest_slot(const Collapse& c, const Slots<N>& s, int S) {
    int h1 = -(1 << 20), h2 = -(1 << 20), at1 = -1;              // a slot without others passes whatever S
    if (Limited) {
#pragma unroll
        for (int q = 0; q < N; q++)
            if (q < s.count) {
                const bool top = s.h[q] > h1;
                h2 = top ? h1 : max(h2, s.h[q]);
                at1 = top ? q : at1;
                h1 = top ? s.h[q] : h1;
            }
    }
    int best = -1;
    float top = -1.0f;
#pragma unroll
    for (int q = 0; q < N; q++)
        if (q < s.count && s.area[q] > top && (!Limited || S + s.count + (q == at1 ? h2 : h1) <= c.limit)) { top = s.area[q]; best = q; }
    return best;
}

template <int N> __device__ __forceinline__ int slot_ref(const Slots<N>& s, int j) {
    int ref = 0;
#pragma unroll
    for (int q = 0; q < N; q++) ref = q == j ? s.ref[q] : ref;
    return ref;
}

// Slot j takes its node's child 0; the node's child 1 becomes the next slot.
template <int N, bool Limited> __device__ __forceinline__ void expand_slot(const Collapse& c, Slots<N>& s, int j) {
    const int node = slot_ref(s, j) - 1;
    set_slot<N, Limited>(c, s, j, node, 0);
    if (c.nodes[node].child[1] != 0) set_slot<N, Limited>(c, s, s.count++, node, 1);
}

// The whole growth of the wide node rooted at r and entered with S.
template <int N, bool Limited> __device__ __forceinline__ void grow(const Collapse& c, Slots<N>& s, int r, int S) {
    first_slots<N, Limited>(c, s, r);
    for (int e = 0; e < N - 1 && s.count < N; e++) {
        const int best = widest_slot<N, Limited>(c, s, S);
        if (best < 0) break;
        expand_slot<N, Limited>(c, s, best);
    }
}

template <int N, bool Limited> __global__ __launch_bounds__(kBlock) void k_collapse_flags(Collapse c) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_nodes) return;
    int flags = 0, is_root = 0;
    const int c0 = c.nodes[i].child[0], c1 = c.nodes[i].child[1];
    // an empty slot is the root's alone (the single-leaf form)
    if (i == 0 ? (c0 == 0 && c1 == 0) : (c0 == 0 || c1 == 0)) flags |= RODENT_BUILD_BAD_TOPOLOGY;
    // up: the turns of the path, the root's in bit 0
    uint64_t turns = 0;
    int depth = 0, at = i;
    while (at != 0 && depth < kMaxClimb) {
        const int up = c.parent[at];
        if (up < 0) break;
        turns = (turns << 1) | (uint64_t)(up & 1);
        at = up >> 1;
        depth++;
    }
    if (at != 0) {
        flags |= RODENT_BUILD_BAD_TOPOLOGY;                       // no way to the root within 64 parents: this node takes no part
    } else if (c.small[i] != 0) {
        // the topmost small node of its path is one packet; the root is a wide node whatever it is
        is_root = i == 0;
        if (i == 0 || c.small[c.parent[i] >> 1] == 0) {
            const int first = c.small_first[i];
            if (first > 0 && !ends_leaf(c, first - 1)) flags |= RODENT_BUILD_BAD_TOPOLOGY;
            else flags |= mark_packet(c, first, c.small[i], true);
        }
    } else {
        if (c0 < 0) flags |= mark_run(c, ~c0);
        if (c1 < 0) flags |= mark_run(c, ~c1);
        // down: through the wide roots above i.  Each one takes at least one turn, so there are at most 64 of them.
        int above = 0;                                            // the sum of (filled slots - 1) over them
        bool inside = false;                                      // i is expanded inside one of them
        for (int w = 0; w < kMaxClimb && at != i && !inside; w++) {
            Slots<N> s;
            first_slots<N, Limited>(c, s, at);
            // the slot on my path: the turn's side (a root without child 0 keeps child 1 in slot 0)
            int on = (int)(turns & 1) != 0 && c.nodes[at].child[0] != 0;
            turns >>= 1; depth--;
            for (int e = 0; e < N - 1 && s.count < N; e++) {
                const int best = widest_slot<N, Limited>(c, s, above);
                if (best < 0) break;
                int next = on;
                if (best == on) {
                    if (depth == 0) { inside = true; break; }     // that slot holds i itself
                    if (turns & 1) next = s.count;
                    turns >>= 1; depth--;
                }
                expand_slot<N, Limited>(c, s, best);
                on = next;
            }
            above += s.count - 1;
            at = slot_ref(s, on) - 1;                             // the wide root my path goes on through (i when depth == 0)
            if ((unsigned)at >= (unsigned)c.num_nodes) inside = true;     // only below a flagged node
        }
        if (!inside && at == i) {
            Slots<N> s;
            grow<N, Limited>(c, s, i, above);
            atomicMax(&c.info[kInfoStackBound], above + s.count - 1);
            if (Limited) c.above[i] = above;
            is_root = 1;
        }
    }
    c.root[i] = is_root;
    if (flags) atomicOr(&c.info[kInfoFlags], flags);
}

// Block totals of (flag & kMarkLanes) != 0 over flag[0, n); k_scan makes them offsets; k_collapse_ids then numbers the flagged items.
__global__ __launch_bounds__(kBlock) void k_collapse_totals(const int* __restrict__ flag, int n, uint32_t* __restrict__ blocktot) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int count = __syncthreads_count(i < n && (flag[i] & kMarkLanes) != 0);
    if (threadIdx.x == 0) blocktot[blockIdx.x] = (uint32_t)count;
}

__global__ __launch_bounds__(kBlock) void k_collapse_ids(const int* __restrict__ flag, int n, const uint32_t* __restrict__ blocktot,
                                                         uint32_t* __restrict__ ids) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_scan(i < n && (flag[i] & kMarkLanes) != 0, &total);
    if (i < n) ids[i] = blocktot[blockIdx.x] + before;
}

__global__ __launch_bounds__(kBlock) void k_collapse_packets(Collapse c, Tri4* __restrict__ packets) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= c.num_bvh_tris) return;
    const int mark = c.mark[p], lanes = mark & kMarkLanes;
    if (lanes == 0) return;
    float col[12][4];
    int prim[4], geom[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool used = k < lanes && p + k < c.num_bvh_tris;
        const float4* rec = reinterpret_cast<const float4*>(c.tris + (used ? p + k : p));
        const float4 a = rec[0], b = rec[1], d = rec[2];
        // n = e1 x e2, every product rounded on its own (the refit's statement)
        const float n[3] = {__fmul_rn(b.y, d.z) - __fmul_rn(b.z, d.y), __fmul_rn(b.z, d.x) - __fmul_rn(b.x, d.z),
                            __fmul_rn(b.x, d.y) - __fmul_rn(b.y, d.x)};
        const float word[12] = {a.x, a.y, a.z, b.x, b.y, b.z, d.x, d.y, d.z, n[0], n[1], n[2]};
#pragma unroll
        for (int r = 0; r < 12; r++) col[r][k] = used ? word[r] : 0.0f;
        prim[k] = used ? __float_as_int(d.w) & 0x7FFFFFFF : -1;
        geom[k] = used ? __float_as_int(b.w) : 0;
    }
    if (mark & kMarkLast) prim[3] |= (int)kLastInLeaf;
    float4* out = reinterpret_cast<float4*>(packets + c.packet_id[p]);
#pragma unroll
    for (int r = 0; r < 12; r++) out[r] = make_float4(col[r][0], col[r][1], col[r][2], col[r][3]);
    reinterpret_cast<int4*>(out)[12] = make_int4(prim[0], prim[1], prim[2], prim[3]);
    reinterpret_cast<int4*>(out)[13] = make_int4(geom[0], geom[1], geom[2], geom[3]);
}

template <class Node, bool Limited> __global__ __launch_bounds__(kBlock) void k_collapse_nodes(Collapse c, Node* __restrict__ wide) {
    constexpr int N = kArity<Node>;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_nodes || c.root[i] == 0) return;
    Node& out = wide[c.wide_id[i]];
    const bool whole = c.small[i] != 0;                           // node 0 only: the whole tree is one packet
    Slots<N> s;
    if (whole) s.count = 0; else grow<N, Limited>(c, s, i, Limited ? c.above[i] : 0);
#pragma unroll
    for (int q = 0; q < N; q++) {
        if (whole && q == 0) {
            // one slot over the union of the root's two boxes (an empty slot's (+inf, -inf) drops out by itself)
            float u[6];
            unite(u, c.nodes[i].bounds, c.nodes[i].bounds + 6);
            for (int j = 0; j < 6; j++) out.bounds[j][0] = u[j];
            out.child[0] = ~(int)c.packet_id[c.small_first[i]];
        } else if (q < s.count) {
            const int ref = s.ref[q];
            const float* b = c.nodes[s.src[q] >> 1].bounds + 6 * (s.src[q] & 1);
            for (int j = 0; j < 6; j++) out.bounds[j][q] = b[j];
            int child = 0;                                        // only below a flagged node
            if (ref < 0) { if (~ref < c.num_bvh_tris) child = ~(int)c.packet_id[~ref]; }
            else if (ref > 0 && ref <= c.num_nodes)
                child = c.small[ref - 1] != 0 ? ~(int)c.packet_id[c.small_first[ref - 1]] : (int)c.wide_id[ref - 1] + 1;
            out.child[q] = child;
        } else {
            for (int j = 0; j < 6; j++) out.bounds[j][q] = j & 1 ? -INFINITY : INFINITY;
            out.child[q] = 0;
        }
        out.pad[q] = 0;
    }
}
