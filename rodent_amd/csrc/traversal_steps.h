// traversal_steps.h -- the BVH2 / Tri1 steps that more than one translation unit walks with: the leaf, the node step, and what the
// instanced loops add to them (the 64-entry LDS stack of both levels, the ray carried into an object's space).  traversal.hip builds
// k_instanced from them (traversal_instanced.h), render.hip the renderer's k_trace_instanced (render_instanced.h): one statement of the
// arithmetic for both.
#pragma once
#include "traversal_device.h"

namespace rodent_dev {

// HitAcc with the accepted Tri1's geom_id beside it (the renderer's hit record holds it)
struct HitAccGeom : HitAcc { int geom; };

// One leaf of Tri1 records (mapping_gpu.impala:156-174).  Returns true when an
// any-hit query is finished.
// WIDE = false: 32-bit byte offsets from a uniform base (global_load ... v_off, s[base:base+1]: one VALU
// instruction of address arithmetic per step instead of two 64-bit ones); the host picks WIDE = true when an
// array is 4 GiB or larger.
template <bool ANY, bool WIDE = true, typename Acc = HitAcc>
__device__ __forceinline__ bool leaf_tri1(const Tri1* __restrict__ tris, int first, RayX& ray, Acc& hit) {
    int j = first;
    for (;;) {
        const float4* p = WIDE ? reinterpret_cast<const float4*>(tris + j)
                               : reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + (unsigned)j
                                   * (unsigned)sizeof(Tri1));
        j++;
        const float4 a = p[0], b = p[1], c = p[2];
        const int prim_id = __float_as_int(c.w);
        const float nx = cross_x(b.x, b.y, b.z, c.x, c.y, c.z);       // mapping_gpu.impala:57
        const float ny = cross_y(b.x, b.y, b.z, c.x, c.y, c.z);
        const float nz = cross_z(b.x, b.y, b.z, c.x, c.y, c.z);
        float t, u, v;
        if (intersect_tri(ray, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, nx, ny, nz, t, u, v)) {
            hit.id = prim_id & 0x7FFFFFFF; hit.t = t; hit.u = u; hit.v = v;
            if constexpr (sizeof(Acc) > sizeof(HitAcc)) hit.geom = __float_as_int(b.w);      // Tri1::geom_id
            ray.tmax = t;
            if (ANY) return true;
        }
        if (prim_id < 0) return false;                                // sentinel (:63,172)
    }
}

// One BVH2 node step (mapping_gpu.impala:107-134): returns the new top; pushes at most one entry.
template <typename Stack>
__device__ __forceinline__ int node2_step(const Node2* __restrict__ nodes, int top, const RayX& ray, Stack& st, int& ptr) {
    const float4* p = reinterpret_cast<const float4*>(nodes + (top - 1));
    const float4 b0 = p[0], b1 = p[1], b2 = p[2];
    const int4 ch = *reinterpret_cast<const int4*>(p + 3);
    float te0, te1;
    // Empty slots (child 0, bounds +inf/-inf) are never taken: the unordered min/max test would
    // turn the inverted box into an infinite one and push node id 0 (= "stack empty").
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

// The 64 entries of one lane of an instanced loop, [entry][lane] in LDS: indices clamped as in DeepStack; an overflow shows in the
// caller's cursor (ptr >= kStackCap), not in a flag.
struct InstanceStack {
    lds_int* base;
    __device__ __forceinline__ void put(int e, int v) { if (e < kStackCap) base[e * kWave] = v; }
    __device__ __forceinline__ int  get(int e) const { return base[(e < kStackCap ? e : kStackCap - 1) * kWave]; }
};

// The ray in the object space of the instance whose world_to_object rows are w0 w1 w2; tmin and the current tmax are shared.
__device__ __forceinline__ RayX object_ray(const RayX& r, const float4& w0, const float4& w1, const float4& w2) {
    RayX o;
    o.ox = ((w0.x * r.ox + w0.y * r.oy) + w0.z * r.oz) + w0.w;
    o.oy = ((w1.x * r.ox + w1.y * r.oy) + w1.z * r.oz) + w1.w;
    o.oz = ((w2.x * r.ox + w2.y * r.oy) + w2.z * r.oz) + w2.w;
    o.dx = (w0.x * r.dx + w0.y * r.dy) + w0.z * r.dz;
    o.dy = (w1.x * r.dx + w1.y * r.dy) + w1.z * r.dz;
    o.dz = (w2.x * r.dx + w2.y * r.dy) + w2.z * r.dz;
    o.idx = safe_rcp(o.dx); o.idy = safe_rcp(o.dy); o.idz = safe_rcp(o.dz);
    o.iox = -(o.ox * o.idx); o.ioy = -(o.oy * o.idy); o.ioz = -(o.oz * o.idz);
    o.tmin = r.tmin; o.tmax = r.tmax;
    return o;
}

} // namespace rodent_dev
