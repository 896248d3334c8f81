// build_motion.h -- the fuse stage of deforming meshes under motion (rules: include/rodent_motion.h; included by bvh_build.hip after
// build_refit.h).  CPU model: tests/motion_bvh_model.py (fuse).
#pragma once
// ---- fuse: two hierarchies of one topology -> RodentMotionNode2 / RodentMotionTri1 ----------------------------------------------------
// Elementwise: thread i < num_nodes makes node record i, the threads behind them one triangle record each.  Every input record is read
// with 16-byte loads and every output record written with 16-byte stores; nothing depends on another thread.
constexpr float kMotionWiden = 1.0f / 524288.0f;        // 2^-19

// `refit_info`: null for the plain fuse; for the build, the info words of its two refits, A's four then B's four: the first thread folds
// them into info ([0] A's node count, [2] |= both flags, [3] B's node count).
__global__ __launch_bounds__(kBlock) void k_fuse_motion(const Node2* __restrict__ nodes0, const Tri1* __restrict__ tris0,
                                                        const Node2* __restrict__ nodes1, const Tri1* __restrict__ tris1, int num_nodes,
                                                        int num_bvh_tris, RodentMotionNode2* __restrict__ motion_nodes,
                                                        RodentMotionTri1* __restrict__ motion_tris,
                                                        const int* __restrict__ refit_info, int* info) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    int flags = 0;
    bool done = false;
    if (i < num_nodes) {
        const float4* p0 = reinterpret_cast<const float4*>(nodes0 + i);
        const float4* p1 = reinterpret_cast<const float4*>(nodes1 + i);
        const float4 a0 = p0[0], a1 = p0[1], a2 = p0[2], b0 = p1[0], b1 = p1[1], b2 = p1[2];
        const int4 w0 = *reinterpret_cast<const int4*>(p0 + 3), w1 = *reinterpret_cast<const int4*>(p1 + 3);
        if (w0.x != w1.x || w0.y != w1.y) flags |= RODENT_BUILD_BAD_TOPOLOGY;      // the record takes key 0's words
        float k0[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        float k1[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
        const int child[2] = {w0.x, w0.y};
        for (int k = 0; k < 2; k++) {
            if (child[k] == 0) continue;                 // an empty slot keeps its (+inf, -inf): inf - inf would be a NaN
            for (int a = 0; a < 3; a++) {
                const int lo = 6 * k + 2 * a, hi = lo + 1;
                const float m = fmaxf(fmaxf(fabsf(k0[lo]), fabsf(k0[hi])), fmaxf(fabsf(k1[lo]), fabsf(k1[hi])));
                const float e = __fmul_rn(kMotionWiden, m);
                k0[lo] = __fsub_rn(k0[lo], e); k0[hi] = __fadd_rn(k0[hi], e);
                k1[lo] = __fsub_rn(k1[lo], e); k1[hi] = __fadd_rn(k1[hi], e);
            }
        }
        float4* out = reinterpret_cast<float4*>(motion_nodes + i);
        for (int q = 0; q < 3; q++) {
            out[q] = make_float4(k0[4 * q], k0[4 * q + 1], k0[4 * q + 2], k0[4 * q + 3]);
            out[3 + q] = make_float4(k1[4 * q], k1[4 * q + 1], k1[4 * q + 2], k1[4 * q + 3]);
        }
        *reinterpret_cast<int4*>(out + 6) = w0;          // child[2], then key 0's two pad words
        *reinterpret_cast<int4*>(out + 7) = make_int4(0, 0, 0, 0);
        done = true;
    } else if (i - num_nodes < num_bvh_tris) {
        const long long p = i - num_nodes;
        const float4* p0 = reinterpret_cast<const float4*>(tris0 + p);
        const float4* p1 = reinterpret_cast<const float4*>(tris1 + p);
        float4* out = reinterpret_cast<float4*>(motion_tris + p);
        for (int q = 0; q < 3; q++) {
            const float4 a = p0[q], b = p1[q];
            if (__float_as_int(a.w) != __float_as_int(b.w)) flags |= RODENT_BUILD_BAD_TOPOLOGY;
            out[q] = a;
            out[3 + q] = make_float4(b.x, b.y, b.z, 0.0f);
        }
        done = true;
    }
    if (i == 0 && refit_info) {
        flags |= refit_info[kInfoFlags] | refit_info[RODENT_BUILD_INFO_WORDS + kInfoFlags];
        info[0] = refit_info[kInfoRefitNodes];
        info[3] = refit_info[RODENT_BUILD_INFO_WORDS + kInfoRefitNodes];
    }
    if (flags) atomicOr(&info[kInfoFlags], flags);
    const int count = __syncthreads_count(done);
    if (threadIdx.x == 0 && count) atomicAdd(&info[1], count);
}
