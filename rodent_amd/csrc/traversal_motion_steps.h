// traversal_motion_steps.h -- the steps over two-key records (include/rodent_motion.h) that more than one translation unit walks with:
// the interpolation of one value, the node step and the leaf.  traversal.hip builds k_bvh2_motion from them (traversal_motion.h),
// render.hip the renderer's k_trace_deforming (render_deforming.h): one statement of the arithmetic for both, as traversal_steps.h is
// for the static records.  CPU model: tests/motion_bvh_model.py.
//
// A step reads one record, interpolates it to the ray's time (s = 1 - t; x = s*x0 + t*x1, every operation rounded on its own) and hands
// the result to the body of the static step (traversal_steps.h: node2_step, leaf_tri1), so whatever the static kernels compute from a
// record, these compute from the interpolated record.  Those bodies are stated a SECOND time here, word for word (motion_node2_pick,
// motion_tri1_test): cut out of node2_step / leaf_tri1 as functions that both forms call, they changed the register rows of kernels
// that existed (k_bvh2_top_persist, k_bvh2_top_auto, k_bvh2_finish, k_instanced, the renderer's k_trace_instanced among them), and those
// kernels keep their code.
// The loads of a record are all issued before the first use: the seven (six) addresses are one base plus immediate offsets, the
// interpolations below them need both keys of a value, so the compiler has nothing to wait for in between.  A node record is one
// 128-byte line; a triangle record is 96 bytes, so two of three straddle a line.
#pragma once
#include "rodent_motion.h"
#include "traversal_steps.h"

namespace rodent_dev {

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

// The body of leaf_tri1 behind its loads: one Tri1 (rows a b c) against the ray; an accepted hit is taken and shortens the ray.  An
// accumulator with a geom word (HitAccGeom, the renderer's hit record) takes the Tri1's geom_id too, as leaf_tri1's does.
template <typename Acc>
__device__ __forceinline__ bool motion_tri1_test(const float4& a, const float4& b, const float4& c, RayX& ray, Acc& hit) {
    const float nx = cross_x(b.x, b.y, b.z, c.x, c.y, c.z);           // mapping_gpu.impala:57
    const float ny = cross_y(b.x, b.y, b.z, c.x, c.y, c.z);
    const float nz = cross_z(b.x, b.y, b.z, c.x, c.y, c.z);
    float t, u, v;
    if (!intersect_tri(ray, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, nx, ny, nz, t, u, v)) return false;
    hit.id = __float_as_int(c.w) & 0x7FFFFFFF; hit.t = t; hit.u = u; hit.v = v;
    if constexpr (sizeof(Acc) > sizeof(HitAcc)) hit.geom = __float_as_int(b.w);      // Tri1::geom_id (key 0's)
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
template <bool ANY, typename Acc = HitAcc>
__device__ __forceinline__ bool leaf_motion_tri1(const RodentMotionTri1* __restrict__ tris, int first, RayX& ray, float s, float t,
                                                 Acc& hit) {
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

} // namespace rodent_dev
