// traversal_instanced.h -- instanced scenes (include/rodent_instances.h; included by traversal.hip inside its namespace): a TLAS of Node2
// records over RodentInstance records, each naming one object's BVH2 / Tri1 inside the packed arrays.  CPU model: tests/instance_model.py.
//
// k_instanced<ANY>: one ray per lane, one 64-ray chunk per one-wave workgroup; the while-while loop of the follow-up kernel (finish_launch)
// on both levels, built from node2_step and leaf_tri1 as they stand.  One stack of the reference's 64 entries serves both levels,
// [entry][lane] in 16 KB of LDS as in k_bvh2_finish (consecutive lanes on consecutive banks): 10 waves per CU of 160 KB.  The whole
// capacity lives in LDS -- no window, no spill path, no follow-up launch -- because the two levels add up: a TLAS over 2^22 instances is up
// to 52 levels deep and an object up to 56, so a ray's real need is decided by the scene, and the contract (a ray whose P + 2 <= 64 is
// traced without a flag) must hold whatever it is.  A smaller window with a spill path would raise the occupancy; it was not built, so
// what it would gain is not known.  DESIGN 11 holds what this form measures against the same geometry baked flat.
// Stack slots, bottom up: 0 (ends the traversal), the TLAS entries -- the continuation of the leaf being visited stays ON the stack while
// its instances are traced, so it costs no register --, 0 (ends the object's traversal), the object's entries.  A push past slot 63
// leaves the cursor above 63: the ray raises the overflow word of the launch context (Ctl::host_err, read by rodent_hip_check_errors),
// stops where it stands and stores whatever hit it holds -- it never pops a slot it did not write.
// The world ray is NOT kept through an object's traversal: every iteration of the kernel's one loop -- a TLAS step or a whole instance --
// loads its 32 bytes again (an L1 / L2 hit) behind an opaque copy of the ray index, so that the compiler cannot keep an earlier load's
// registers alive instead; only tmax, which both spaces share, is carried.  (Written as nested loops with the ray assigned again behind
// each object, the compiler kept the ray's slab operands in 32 bytes of scratch per lane.)  That is more often than needed: a TLAS step
// that follows a TLAS step loads the ray and takes its three reciprocals again; what that costs has not been measured apart.
#pragma once

// InstanceStack (the 64 entries of one lane) and object_ray (the ray in an instance's object space): traversal_steps.h.

template <bool ANY>
__global__ __launch_bounds__(kWave) void k_instanced(const Node2* __restrict__ tlas, const RodentInstance* __restrict__ instances,
                                                     const Node2* __restrict__ nodes, const Tri1* __restrict__ tris,
                                                     const Ray1* __restrict__ rays, Hit1* __restrict__ hits,
                                                     int* __restrict__ hit_instances, int n, Ctl* ctl) {
    __shared__ int stack_lds[kStackCap * kWave];
    const int i = blockIdx.x * kWave + threadIdx.x;
    if (i >= n) return;
    InstanceStack st{(lds_int*)stack_lds + threadIdx.x};
    float tmax = reinterpret_cast<const float4*>(rays + i)[1].w;
    HitAcc hit{-1, tmax, 0.0f, 0.0f};
    int hit_instance = -1;
    int ptr = 0, top = 1; st.put(0, 0);
    int j = -1;                                                         // the instance to enter next, -1: a TLAS step is next
    bool overflow = false;
    // One loop for both levels: an iteration is one TLAS step (j < 0) or one whole instance (j >= 0).  The world ray is a local of the
    // iteration, loaded behind an opaque copy of the ray index, so no register holds it across an object's traversal.
    while (top != 0) {
        int again = i;
        asm volatile("" : "+v"(again));
        RayX ray = load_ray(rays, again);
        ray.tmax = tmax;
        if (j < 0) {
            top = node2_step(tlas, top, ray, st, ptr);
            if (ptr >= kStackCap) { overflow = true; break; }
            if (top < 0) j = ~top;                                      // a TLAS leaf: its continuation stays in slot ptr
            continue;
        }
        const float4* p = reinterpret_cast<const float4*>(instances + j);
        const float4 w0 = p[0], w1 = p[1], w2 = p[2];
        const int4 id = *reinterpret_cast<const int4*>(p + 3);          // node_offset, tri_offset, instance_id, pad
        RayX o = object_ray(ray, w0, w1, w2);
        const Node2* onodes = nodes + id.x;
        const Tri1* otris = tris + id.y;
        HitAcc h{-1, 0.0f, 0.0f, 0.0f};
        bool done = false;
        int otop = 1; st.put(++ptr, 0);
        if (ptr >= kStackCap) { overflow = true; break; }
        while (otop != 0) {
            otop = node2_step(onodes, otop, o, st, ptr);
            if (ptr >= kStackCap) { overflow = true; break; }
            while (otop < 0) {
                const int first = ~otop; otop = st.get(ptr); ptr--;
                if (leaf_tri1<ANY>(otris, first, o, h)) { done = true; otop = 0; break; }
            }
        }
        if (h.id >= 0) { hit = h; hit_instance = id.z & 0x7FFFFFFF; }
        if (overflow || (ANY && done)) break;
        tmax = o.tmax;
        j++;
        if (id.z < 0) {                                                 // the last instance of the leaf: on with its continuation
            top = st.get(ptr); ptr--;
            j = top < 0 ? ~top : -1;
        }
    }
    if (overflow) __hip_atomic_store(ctl->host_err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    store_hit(hits, i, hit.id, hit.t, hit.u, hit.v);
    if (hit_instances) hit_instances[i] = hit_instance;
}
