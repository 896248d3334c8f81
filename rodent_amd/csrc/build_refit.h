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
