// traversal_motion.h -- deforming meshes under motion (include/rodent_motion.h; included by traversal.hip inside its namespace): a BVH2
// whose records hold two keys, the mesh at time 0 and at time 1, and a time per ray.  CPU model: tests/motion_bvh_model.py.
//
// k_bvh2_motion<ANY>: one ray per lane, one 64-ray chunk per one-wave workgroup, the while-while loop and the schedule of k_instanced
// (traversal_instanced.h) on one level: the whole stack of the reference's 64 entries as [entry][lane] in 16 KB of LDS (InstanceStack),
// no window, no spill path, no follow-up launch -- 10 waves per CU of 160 KB.  A step reads one record, interpolates it to the ray's
// time (s = 1 - t; x = s*x0 + t*x1, every operation rounded on its own) and hands the result to the body of the static step
// (traversal_steps.h: node2_step, leaf_tri1), so whatever the static kernels compute from a record, this one computes from the
// interpolated record.  Those bodies are stated a SECOND time here, word for word (motion_node2_pick, motion_tri1_test): cut out of
// node2_step / leaf_tri1 as functions that both forms call, they changed the register rows of kernels that existed (k_bvh2_top_persist,
// k_bvh2_top_auto, k_bvh2_finish, k_instanced, the renderer's k_trace_instanced among them), and those kernels keep their code.
// s and t are taken once per ray and live in two registers through the loop.
// The loads of a record are all issued before the first use: the seven (six) addresses are one base plus immediate offsets, the
// interpolations below them need both keys of a value, so the compiler has nothing to wait for in between.  A node record is one
// 128-byte line; a triangle record is 96 bytes, so two of three straddle a line.
#pragma once

// One value at the ray's time: two products and a sum.
__device__ __forceinline__ float lerp_key(float s, float t, float x0, float x1) {
    return __fadd_rn(__fmul_rn(s, x0), __fmul_rn(t, x1));
}
__device__ __forceinline__ float4 lerp_row(float s, float t, const float4& k0, const float4& k1) {
    return make_float4(lerp_key(s, t, k0.x, k1.x), lerp_key(s, t, k0.y, k1.y), lerp_key(s, t, k0.z, k1.z), lerp_key(s, t, k0.w, k1.w));
}

// The body of node2_step behind its loads (mapping_gpu.impala:107-134): returns the new top; pushes at most one entry.
template <typename Stack>
__device__ __forceinline__ int motion_node2_pick(const float4& b0, const float4& b1, const float4& b2, const int4& ch, const RayX& ray,
                                                 Stack& st, int& ptr) {
    float te0, te1;
    // Empty slots (child 0) are never taken, whatever their interpolated bounds are.
    const bool h0 = slab(ray, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, te0) && ch.x != 0;
    const bool h1 = slab(ray, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, te1) && ch.y != 0;
    if (!h0 && !h1) { const int t = st.get(ptr); ptr--; return t; }
    if (h0 && h1) {
        const bool c0first = te0 < te1;                               // strict <  (:128-129)
        st.put(++ptr, c0first ? ch.y : ch.x);
        return c0first ? ch.x : ch.y;
    }
    return h0 ? ch.x : ch.y;
}

// The body of leaf_tri1 behind its loads: one Tri1 (rows a b c) against the ray; an accepted hit is taken and shortens the ray.
__device__ __forceinline__ bool motion_tri1_test(const float4& a, const float4& b, const float4& c, RayX& ray, HitAcc& hit) {
    const float nx = cross_x(b.x, b.y, b.z, c.x, c.y, c.z);           // mapping_gpu.impala:57
    const float ny = cross_y(b.x, b.y, b.z, c.x, c.y, c.z);
    const float nz = cross_z(b.x, b.y, b.z, c.x, c.y, c.z);
    float t, u, v;
    if (!intersect_tri(ray, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, nx, ny, nz, t, u, v)) return false;
    hit.id = __float_as_int(c.w) & 0x7FFFFFFF; hit.t = t; hit.u = u; hit.v = v;
    ray.tmax = t;
    return true;
}

// One node step over a two-key record: seven loads, 24 interpolations, the body of node2_step.
template <typename Stack>
__device__ __forceinline__ int motion_node2_step(const RodentMotionNode2* __restrict__ nodes, int top, const RayX& ray, float s, float t,
                                                 Stack& st, int& ptr) {
    const float4* p = reinterpret_cast<const float4*>(nodes + (top - 1));
    const float4 a0 = p[0], a1 = p[1], a2 = p[2], c0 = p[3], c1 = p[4], c2 = p[5];
    const int4 ch = *reinterpret_cast<const int4*>(p + 6);
    return motion_node2_pick(lerp_row(s, t, a0, c0), lerp_row(s, t, a1, c1), lerp_row(s, t, a2, c2), ch, ray, st, ptr);
}

// One leaf of two-key records: six loads, nine interpolations, the body of leaf_tri1 with key 0's w words.  Returns true when an any-hit query is
// finished.
template <bool ANY>
__device__ __forceinline__ bool leaf_motion_tri1(const RodentMotionTri1* __restrict__ tris, int first, RayX& ray, float s, float t,
                                                 HitAcc& hit) {
    int j = first;
    for (;;) {
        const float4* p = reinterpret_cast<const float4*>(tris + j);
        j++;
        const float4 a0 = p[0], b0 = p[1], c0 = p[2], a1 = p[3], b1 = p[4], c1 = p[5];
        const float4 a = make_float4(lerp_key(s, t, a0.x, a1.x), lerp_key(s, t, a0.y, a1.y), lerp_key(s, t, a0.z, a1.z), a0.w);
        const float4 b = make_float4(lerp_key(s, t, b0.x, b1.x), lerp_key(s, t, b0.y, b1.y), lerp_key(s, t, b0.z, b1.z), b0.w);
        const float4 c = make_float4(lerp_key(s, t, c0.x, c1.x), lerp_key(s, t, c0.y, c1.y), lerp_key(s, t, c0.z, c1.z), c0.w);
        if (motion_tri1_test(a, b, c, ray, hit) && ANY) return true;
        if (__float_as_int(c0.w) < 0) return false;                   // key 0's prim word: bit 31 = the last of the leaf
    }
}

template <bool ANY>
__global__ __launch_bounds__(kWave) void k_bvh2_motion(const RodentMotionNode2* __restrict__ nodes,
                                                       const RodentMotionTri1* __restrict__ tris, const Ray1* __restrict__ rays,
                                                       const float* __restrict__ times, Hit1* __restrict__ hits, int n, Ctl* ctl) {
    __shared__ int stack_lds[kStackCap * kWave];
    const int i = blockIdx.x * kWave + threadIdx.x;
    if (i >= n) return;
    InstanceStack st{(lds_int*)stack_lds + threadIdx.x};
    RayX ray = load_ray(rays, i);
    const float t = times[i];
    HitAcc hit{-1, ray.tmax, 0.0f, 0.0f};
    bool overflow = false;
    // The time rule: a ray outside [0, 1] (a NaN fails both comparisons) is a miss as it stands: its lane sits out the loop beside its
    // traced neighbours.
    if (0.0f <= t && t <= 1.0f) {
        const float s = __fsub_rn(1.0f, t);
        int ptr = 0, top = 1; st.put(0, 0);
        while (top != 0) {
            top = motion_node2_step(nodes, top, ray, s, t, st, ptr);
            if (ptr >= kStackCap) { overflow = true; break; }           // the 64th push was not stored: stop where it stands
            while (top < 0) {
                const int first = ~top; top = st.get(ptr); ptr--;
                if (leaf_motion_tri1<ANY>(tris, first, ray, s, t, hit)) { top = 0; break; }
            }
        }
    }
    if (overflow) __hip_atomic_store(ctl->host_err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    store_hit(hits, i, hit.id, hit.t, hit.u, hit.v);
}
