// build_refit.h -- the refit kernels of the device BVH builder (included by bvh_build.hip after build_split.h).
#pragma once
// ---- refit: the boxes and Tri1 records of an existing hierarchy from moved vertices (rules: include/rodent_build.h) --------------
// The topology (child, pad and w words) is read and never written.  k_refit_links gives every inner child its parent slot, k_refit_tris
// rewrites the records and leaves their boxes in scratch, k_refit_climb fills the boxes bottom-up.  A node is complete after
// 1 + (children with id > 0) arrivals at its counter: its own thread's, once its leaf slots are filled, and one per inner child.  The
// last arriver unions the node's 12 bounds into its slot of the parent and arrives there; nobody waits for anybody, and since every
// value of a counter is returned once, a node is completed at most once: a malformed tree (a cycle, a child id out of range, a child
// claimed twice) leaves nodes incomplete, never a thread looping or a read out of bounds.
enum { kInfoRefitNodes = 0, kInfoRefitTris = 1 };

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
                unite(b, b, tribox + 6 * (size_t)p);
                ended = tris[p].prim_id < 0;
            }
            if (ended) for (int j = 0; j < 6; j++) nodes[node].bounds[6 * k + j] = b[j];
            else atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);       // a leaf without an end bit
        }
    }
    bool active = node >= 0;
    int completed = 0;
    // the wave-uniform form of the hand-off (build_device.h)
    for (int step = 0; step <= num_nodes; step++) {
        if (__ballot(active) == 0) break;
        publish();
        bool last = false;
        if (active) {
            const uint32_t needed = 1u + (nodes[node].child[0] > 0) + (nodes[node].child[1] > 0);
            last = arrive(&arrivals[node]) == needed - 1u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        active = false;
        if (last) {
            completed++;
            const int up = parent[node];
            if (up >= 0) {
                const float* b = nodes[node].bounds;
                float u[6];
                unite(u, b, b + 6);
                node = up >> 1;
                for (int j = 0; j < 6; j++) nodes[node].bounds[6 * (up & 1) + j] = u[j];
                active = true;
            }
        }
    }
    completed = wave_sum(completed);
    if (lane_id() == 0 && completed) atomicAdd(&info[kInfoRefitNodes], completed);
}

// ---- the same for Node4 / Node8 + Tri4 (rules: include/rodent_build.h, "refit of the wide layouts") ---------------------------------
// Three launches again: k_refit_wide_links (parent slot N * i + k), k_refit_tri4 (the valid lanes' columns and the packets' boxes),
// k_refit_wide_climb (leaf slots from the packet boxes, then k_refit_climb's hand-off with N slots to a node).
template <class Node> constexpr int kArity = sizeof(Node::child) / sizeof(int32_t);

// Children of `nd` with an id > 0: its inner slots, sound or not.
template <class Node> __device__ __forceinline__ uint32_t inner_slots(const Node& nd) {
    uint32_t inner = 0;
    for (int k = 0; k < kArity<Node>; k++) inner += nd.child[k] > 0;
    return inner;
}

template <class Node>
__global__ __launch_bounds__(kBlock) void k_refit_wide_links(const Node* __restrict__ nodes, int num_nodes, int num_packets, int* parent,
                                                             uint32_t* __restrict__ arrivals, int* info) {
    constexpr int N = kArity<Node>;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= num_nodes) return;
    arrivals[i] = 0u;
    int flags = 0;
    for (int k = 0; k < N; k++) {
        const int c = nodes[i].child[k];
        if (c > 0) {
            // node 0 is the root: nobody's child.  A child that already has a parent slot keeps it.
            if (c > num_nodes || c == 1 || atomicCAS(&parent[c - 1], -1, N * i + k) != -1) flags |= RODENT_BUILD_BAD_TOPOLOGY;
        } else if (c < 0 && ~c >= num_packets) {
            flags |= RODENT_BUILD_BAD_TOPOLOGY;
        }
    }
    if (flags) atomicOr(&info[kInfoFlags], flags);
}

// Four adjacent threads to a packet, one to a lane: a row of the packet is one 16-byte piece across them.  They share a wave, so the
// packet's box is two __shfl_xor steps away; every thread of the block reaches the shuffles.
__global__ __launch_bounds__(kBlock) void k_refit_tri4(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                       int num_tris, Tri4* __restrict__ tris, int num_packets, float* __restrict__ pbox,
                                                       int* info) {
    const int p = blockIdx.x * (kBlock / 4) + (threadIdx.x >> 2), lane = threadIdx.x & 3;
    float box[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
    bool done = false;
    if (p < num_packets) {
        Tri4& q = tris[p];
        const int4 id = *reinterpret_cast<const int4*>(q.prim_id);
        // the traversal kernels' rule: the first -1 ends the packet
        const bool valid = id.x != -1 && (lane < 1 || id.y != -1) && (lane < 2 || id.z != -1) && (lane < 3 || id.w != -1);
        const int t = (lane == 0 ? id.x : lane == 1 ? id.y : lane == 2 ? id.z : id.w) & 0x7FFFFFFF;
        if (valid && t < num_tris) {
            float3 v[3]; int geom;
            load_triangle(vertices, nv, indices, t, v, &geom, info);
            const TriGeometry g = tri1_geometry(v);
            // n = e1 x e2 as host/vec.h's cross: every product rounded on its own, no fused multiply-add
            const float nx = __fmul_rn(g.e1.y, g.e2.z) - __fmul_rn(g.e1.z, g.e2.y);
            const float ny = __fmul_rn(g.e1.z, g.e2.x) - __fmul_rn(g.e1.x, g.e2.z);
            const float nz = __fmul_rn(g.e1.x, g.e2.y) - __fmul_rn(g.e1.y, g.e2.x);
            q.v0[0][lane] = g.v0.x; q.v0[1][lane] = g.v0.y; q.v0[2][lane] = g.v0.z;
            q.e1[0][lane] = g.e1.x; q.e1[1][lane] = g.e1.y; q.e1[2][lane] = g.e1.z;
            q.e2[0][lane] = g.e2.x; q.e2[1][lane] = g.e2.y; q.e2[2][lane] = g.e2.z;
            q.n[0][lane] = nx; q.n[1][lane] = ny; q.n[2][lane] = nz;
            triangle_box(v, box);
            done = true;
        } else if (valid) {
            atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);      // the lane stays as it is, its box is empty
        }
    }
    for (int w = 1; w <= 2; w <<= 1)
        for (int a = 0; a < 3; a++) {
            box[2 * a] = fminf(box[2 * a], __shfl_xor(box[2 * a], w));
            box[2 * a + 1] = fmaxf(box[2 * a + 1], __shfl_xor(box[2 * a + 1], w));
        }
    if (p < num_packets && lane == 0)
        for (int k = 0; k < 6; k++) pbox[6 * (size_t)p + k] = box[k];
    const int count = __syncthreads_count(done);
    if (threadIdx.x == 0 && count) atomicAdd(&info[kInfoRefitTris], count);
}

template <class Node>
__global__ __launch_bounds__(kBlock) void k_refit_wide_climb(Node* nodes, int num_nodes, const Tri4* __restrict__ tris, int num_packets,
                                                             const float* __restrict__ pbox, const int* __restrict__ parent,
                                                             uint32_t* arrivals, int* info) {
    constexpr int N = kArity<Node>;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int node = i < num_nodes ? i : -1;
    if (node >= 0) {
        for (int k = 0; k < N; k++) {
            const int c = nodes[node].child[k];
            if (c >= 0 || ~c >= num_packets) continue;           // empty, inner, or flagged by k_refit_wide_links: the slot stays as stored
            float b[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
            bool ended = false;
            for (int p = ~c; p < num_packets && !ended; p++) {
                unite(b, b, pbox + 6 * (size_t)p);
                ended = tris[p].prim_id[3] < 0;
            }
            if (ended) for (int j = 0; j < 6; j++) nodes[node].bounds[j][k] = b[j];
            else atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);       // a leaf without an end
        }
    }
    bool active = node >= 0;
    int completed = 0;
    // the wave-uniform form of the hand-off (build_device.h), as in k_refit_climb
    for (int step = 0; step <= num_nodes; step++) {
        if (__ballot(active) == 0) break;
        publish();
        bool last = false;
        if (active) last = arrive(&arrivals[node]) == inner_slots(nodes[node]);      // 1 + inner slots arrivals complete it
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        active = false;
        if (last) {
            completed++;
            const int up = parent[node];
            if (up >= 0) {
                float u[6];
                for (int j = 0; j < 6; j++) {                    // rows 0 2 4: the lows, rows 1 3 5: the highs; an empty slot drops out
                    const float* row = nodes[node].bounds[j];
                    u[j] = row[0];
                    for (int k = 1; k < N; k++) u[j] = j & 1 ? fmaxf(u[j], row[k]) : fminf(u[j], row[k]);
                }
                node = up / N;
                for (int j = 0; j < 6; j++) nodes[node].bounds[j][up % N] = u[j];
                active = true;
            }
        }
    }
    completed = wave_sum(completed);
    if (lane_id() == 0 && completed) atomicAdd(&info[kInfoRefitNodes], completed);
}

// ---- the refit of a chosen subset of the packed objects of an instanced scene (rules: include/rodent_instances.h) ------------------
// The three launches of the refit over the listed objects' nodes and records laid end to end: element i of the node space belongs to
// the range r with ranges[r].node_start <= i < ranges[r + 1].node_start (the record space likewise by rec_start), found by a bisection
// of the range table, and works on its object's records at node_offset / tri_offset with object-local ids, in the object's own stretch
// of the scratch arrays (parent and arrivals at node_start, tribox at rec_start).  What a range claims is checked against the totals
// the call was given before anything of it is indexed (forest_span): a range that fails has nothing touched.
struct ForestSpan {
    int node_offset, tri_offset, num_nodes, num_recs;    // the object (RodentObject)
    int first_tri, num_tris;                             // its rows of the index table
    int node_start, rec_start;                           // its stretch of the node and record spaces
    int flags;                                           // 0: sound
};
struct ForestArgs {
    const RodentObject* objects; const RodentRefitRange* ranges;
    int num_objects, num_listed, total_nodes, total_recs, num_rows;
};

__device__ __forceinline__ ForestSpan forest_span(const ForestArgs& a, int r) {
    const RodentRefitRange g = a.ranges[r];
    ForestSpan s{};
    s.first_tri = g.first_tri; s.num_tris = g.num_tris; s.node_start = g.node_start; s.rec_start = g.rec_start;
    if ((unsigned)g.object >= (unsigned)a.num_objects) { s.flags = RODENT_TLAS_BAD_OBJECT; return s; }
    const RodentObject o = a.objects[g.object];
    s.node_offset = o.node_offset; s.tri_offset = o.tri_offset; s.num_nodes = o.num_nodes; s.num_recs = o.num_tris;
    const bool sound = o.num_nodes >= 1 && o.num_tris >= 1 && g.first_tri >= 0 && g.num_tris >= 1 && g.first_tri <= a.num_rows - g.num_tris
        && g.node_start >= 0 && g.node_start <= a.total_nodes - o.num_nodes && g.rec_start >= 0 && g.rec_start <= a.total_recs - o.num_tris;
    if (!sound) s.flags = RODENT_BUILD_BAD_TOPOLOGY;
    return s;
}

// The last range whose start (Records: rec_start, else node_start) is <= i: at most 32 halvings.  An empty range in front of another
// shares its start and loses to it.
template <bool Records> __device__ __forceinline__ int forest_range(const ForestArgs& a, int i) {
    int lo = 0, hi = a.num_listed;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((Records ? a.ranges[mid].rec_start : a.ranges[mid].node_start) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The first num_listed threads also judge one range each: its flag is raised once, whether or not an element falls into it.
__global__ __launch_bounds__(kBlock) void k_forest_links(const Node2* __restrict__ nodes, ForestArgs a, int* parent,
                                                         uint32_t* __restrict__ arrivals, int* info) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int flags = i < a.num_listed ? forest_span(a, i).flags : 0;
    if (i < a.total_nodes) {
        arrivals[i] = 0u;
        const ForestSpan s = forest_span(a, forest_range<false>(a, i));
        const int local = i - s.node_start;
        if (!s.flags && local >= 0 && local < s.num_nodes) {
            for (int k = 0; k < 2; k++) {
                const int c = nodes[s.node_offset + local].child[k];
                if (c > 0) {
                    // local node 0 is its object's root: nobody's child.  A child that already has a parent slot keeps it.
                    if (c > s.num_nodes || c == 1 || atomicCAS(&parent[s.node_start + c - 1], -1, 2 * local + k) != -1)
                        flags |= RODENT_BUILD_BAD_TOPOLOGY;
                } else if (c < 0 && ~c >= s.num_recs) {
                    flags |= RODENT_BUILD_BAD_TOPOLOGY;
                }
            }
        }
    }
    if (flags) atomicOr(&info[kInfoFlags], flags);
}

__global__ __launch_bounds__(kBlock) void k_forest_tris(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                        Tri1* __restrict__ tris, ForestArgs a, float* __restrict__ tribox, int* info) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    bool done = false;
    if (p < a.total_recs) {
        float box[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
        const ForestSpan s = forest_span(a, forest_range<true>(a, p));
        const int local = p - s.rec_start;
        if (!s.flags && local >= 0 && local < s.num_recs) {
            float4* rec = reinterpret_cast<float4*>(tris + s.tri_offset + local);
            const float4 w2 = rec[2];
            const int t = (int)((uint32_t)__float_as_int(w2.w) & ~kLastInLeaf);
            if (t < s.num_tris) {
                float3 v[3]; int geom;
                load_triangle(vertices, nv, indices + s.first_tri, t, v, &geom, info);
                const TriGeometry g = tri1_geometry(v);
                rec[0] = make_float4(g.v0.x, g.v0.y, g.v0.z, rec[0].w);
                rec[1] = make_float4(g.e1.x, g.e1.y, g.e1.z, rec[1].w);
                rec[2] = make_float4(g.e2.x, g.e2.y, g.e2.z, w2.w);
                triangle_box(v, box);
                done = true;
            } else {
                atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);  // the record stays as it is, its box is empty
            }
        }
        for (int k = 0; k < 6; k++) tribox[6 * (size_t)p + k] = box[k];
    }
    const int count = __syncthreads_count(done);
    if (threadIdx.x == 0 && count) atomicAdd(&info[kInfoRefitTris], count);
}

// k_refit_climb with a lane's node, parent slots and counters relative to its object.  A wave may hold nodes of several objects: the
// loop's bound is total_nodes, which no sound range's node count exceeds, and a lane's climb ends at its own object's local node 0.
__global__ __launch_bounds__(kBlock) void k_forest_climb(Node2* nodes, const Tri1* __restrict__ tris, ForestArgs a,
                                                         const float* __restrict__ tribox, const int* __restrict__ parent,
                                                         uint32_t* arrivals, int* info) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int node = -1;
    ForestSpan s{};
    if (i < a.total_nodes) {
        s = forest_span(a, forest_range<false>(a, i));
        const int local = i - s.node_start;
        if (!s.flags && local >= 0 && local < s.num_nodes) node = local;
    }
    Node2* const mine = nodes + s.node_offset;           // the object's nodes, parent slots and counters
    const int* const up_of = parent + s.node_start;
    uint32_t* const arrived = arrivals + s.node_start;
    if (node >= 0) {
        const Tri1* const recs = tris + s.tri_offset;
        const float* const boxes = tribox + 6 * (size_t)s.rec_start;
        for (int k = 0; k < 2; k++) {
            const int c = mine[node].child[k];
            if (c >= 0 || ~c >= s.num_recs) continue;            // empty, inner, or flagged by k_forest_links: the slot stays as stored
            float b[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
            bool ended = false;
            for (int p = ~c; p < s.num_recs && !ended; p++) {
                unite(b, b, boxes + 6 * (size_t)p);
                ended = recs[p].prim_id < 0;
            }
            if (ended) for (int j = 0; j < 6; j++) mine[node].bounds[6 * k + j] = b[j];
            else atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);       // a leaf without an end bit
        }
    }
    bool active = node >= 0, strayed = false;
    int completed = 0;
    // the wave-uniform form of the hand-off (build_device.h), as in k_refit_climb
    for (int step = 0; step <= a.total_nodes; step++) {
        if (__ballot(active) == 0) break;
        publish();
        bool last = false;
        if (active) {
            const uint32_t needed = 1u + (mine[node].child[0] > 0) + (mine[node].child[1] > 0);
            last = arrive(&arrived[node]) == needed - 1u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        active = false;
        if (last) {
            completed++;
            const int up = up_of[node];
            // (a slot beyond the object's nodes: another range's, under a range table that lets two stretches overlap)
            if (up >= 0 && (up >> 1) < s.num_nodes) {
                const float* b = mine[node].bounds;
                float u[6];
                unite(u, b, b + 6);
                node = up >> 1;
                for (int j = 0; j < 6; j++) mine[node].bounds[6 * (up & 1) + j] = u[j];
                active = true;
            } else if (up >= 0) {
                strayed = true;
            }
        }
    }
    if (strayed) atomicOr(&info[kInfoFlags], RODENT_BUILD_BAD_TOPOLOGY);
    completed = wave_sum(completed);
    if (lane_id() == 0 && completed) atomicAdd(&info[kInfoRefitNodes], completed);
}
