// traversal_motion.h -- deforming meshes under motion (include/rodent_motion.h; included by traversal.hip inside its namespace): a BVH2
// whose records hold two keys, the mesh at time 0 and at time 1, and a time per ray.  CPU model: tests/motion_bvh_model.py.
//
// k_bvh2_motion<ANY>: one ray per lane, one 64-ray chunk per one-wave workgroup, the while-while loop and the schedule of k_instanced
// (traversal_instanced.h) on one level: the whole stack of the reference's 64 entries as [entry][lane] in 16 KB of LDS (InstanceStack),
// no window, no spill path, no follow-up launch -- 10 waves per CU of 160 KB.  The steps over a record -- lerp_key, motion_node2_step,
// leaf_motion_tri1 -- are traversal_motion_steps.h's (included by traversal.hip at file scope), which the renderer's
// k_trace_deforming (render_deforming.h) walks with too.
// s and t are taken once per ray and live in two registers through the loop.
#pragma once

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
