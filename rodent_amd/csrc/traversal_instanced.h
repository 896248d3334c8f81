// traversal_instanced.h -- instanced scenes (include/rodent_instances.h; included by traversal.hip inside its namespace): a TLAS of Node2
// records over RodentInstance records, each naming one object's BVH2 / Tri1 inside the packed arrays.  CPU model: tests/instance_model.py.
// k_instanced_motion<ANY> is the same loop over RodentMotionInstance records (two placements each) with a time per ray: the loop is stated
// once, instanced_loop, and the two kernels differ in how a record yields the object ray (StaticEnter, MotionEnter).  CPU model:
// tests/motion_instance_model.py.
// k_instanced_motion_objects<ANY> is that loop again over a motion TLAS whose objects hold two-key records (RodentMotionNode2 /
// RodentMotionTri1): the loop's second policy says how the object level is walked (StaticObjects, MotionObjects), and one time per ray
// serves both levels.  CPU model: tests/motion_objects_model.py.
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

// How an instance record yields the object ray: the one difference between k_instanced and k_instanced_motion.  enter(j, i, ray, o, id)
// reads record j for ray i, fills the object ray and id = {node_offset, tri_offset, instance_id, pad}, and returns whether the instance
// is entered at all.
struct StaticEnter {
    const RodentInstance* instances;
    __device__ __forceinline__ bool enter(int j, int, const RayX& ray, RayX& o, int4& id) const {
        const float4* p = reinterpret_cast<const float4*>(instances + j);
        const float4 w0 = p[0], w1 = p[1], w2 = p[2];
        id = *reinterpret_cast<const int4*>(p + 3);                     // node_offset, tri_offset, instance_id, pad
        o = object_ray(ray, w0, w1, w2);
        return true;
    }
};

// Seven 16-byte loads of the record's one cache line (its last 16 bytes are padding), the ray's time loaded again behind the same opaque index as the ray, 12 interpolations, the fp64
// inverse of the build stage (instance_inverse.h), the skip test, object_ray.
struct MotionEnter {
    const RodentMotionInstance* instances;
    const float* times;
    __device__ __forceinline__ bool enter(int j, int i, const RayX& ray, RayX& o, int4& id) const {
        const float4* p = reinterpret_cast<const float4*>(instances + j);
        float4 r[6];
        for (int k = 0; k < 6; k++) r[k] = p[k];
        id = *reinterpret_cast<const int4*>(p + 6);                     // node_offset, tri_offset, instance_id, pad
        const float m0[12] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w};
        const float m1[12] = {r[3].x, r[3].y, r[3].z, r[3].w, r[4].x, r[4].y, r[4].z, r[4].w, r[5].x, r[5].y, r[5].z, r[5].w};
        float m[12], w[12];
        lerp_affine(m0, m1, times[i], m);
        if (invert_affine(m, w)) return false;                          // singular or non-finite at this ray's time: skipped, no flag
        o = object_ray(ray, make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]),
                       make_float4(w[8], w[9], w[10], w[11]));
        return true;
    }
};

// How the object level is walked: the second policy of the loop.  time(i) is what a ray keeps through the loop, traced() the time rule
// (tested once, before the loop), step / leaf one node / one leaf of the entered object.  StaticObjects: Node2 / Tri1 with node2_step and
// leaf_tri1 as they stand; a ray keeps nothing and is always traced.
struct StaticObjects {
    struct Time {};
    __device__ __forceinline__ Time time(int) const { return {}; }
    __device__ __forceinline__ static bool traced(const Time&) { return true; }
    __device__ __forceinline__ static int step(const Node2* nodes, int top, const RayX& o, const Time&, InstanceStack& st, int& ptr) {
        return node2_step(nodes, top, o, st, ptr);
    }
    template <bool ANY>
    __device__ __forceinline__ static bool leaf(const Tri1* tris, int first, RayX& o, const Time&, HitAcc& h) {
        return leaf_tri1<ANY>(tris, first, o, h);
    }
};

// MotionObjects: RodentMotionNode2 / RodentMotionTri1 (the offsets of an instance record count these records) with motion_node2_step and
// leaf_motion_tri1 at the ray's time.  s = 1 - t and t live in two registers through the loop, as in k_bvh2_motion; the time rule is
// rodent_motion.h's: !(0 <= t && t <= 1), a NaN included, is a miss without any traversal.
struct MotionObjects {
    const float* times;
    struct Time { float s, t; };
    __device__ __forceinline__ Time time(int i) const { const float t = times[i]; return {__fsub_rn(1.0f, t), t}; }
    __device__ __forceinline__ static bool traced(const Time& tm) { return 0.0f <= tm.t && tm.t <= 1.0f; }
    __device__ __forceinline__ static int step(const RodentMotionNode2* nodes, int top, const RayX& o, const Time& tm, InstanceStack& st,
                                               int& ptr) {
        return motion_node2_step(nodes, top, o, tm.s, tm.t, st, ptr);
    }
    template <bool ANY>
    __device__ __forceinline__ static bool leaf(const RodentMotionTri1* tris, int first, RayX& o, const Time& tm, HitAcc& h) {
        return leaf_motion_tri1<ANY>(tris, first, o, tm.s, tm.t, h);
    }
};

// The loop of all three kernels, stated once.
template <bool ANY, class Objects = StaticObjects, class Enter, class ObjNode, class ObjTri>
__device__ __forceinline__ void instanced_loop(const Node2* __restrict__ tlas, const Enter& in, const ObjNode* __restrict__ nodes,
                                               const ObjTri* __restrict__ tris, const Ray1* __restrict__ rays, Hit1* __restrict__ hits,
                                               int* __restrict__ hit_instances, int n, Ctl* ctl, int* stack_lds,
                                               const Objects& objs = Objects{}) {
    const int i = blockIdx.x * kWave + threadIdx.x;
    if (i >= n) return;
    InstanceStack st{(lds_int*)stack_lds + threadIdx.x};
    float tmax = reinterpret_cast<const float4*>(rays + i)[1].w;
    HitAcc hit{-1, tmax, 0.0f, 0.0f};
    int hit_instance = -1;
    int ptr = 0, top = 1; st.put(0, 0);
    int j = -1;                                                         // the instance to enter next, -1: a TLAS step is next
    bool overflow = false;
    const typename Objects::Time tm = objs.time(i);
    if (!Objects::traced(tm)) top = 0;                                  // a refused time: the lane sits out the loop, a miss as it stands
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
        RayX o;
        int4 id;
        if (in.enter(j, again, ray, o, id)) {
            const ObjNode* onodes = nodes + id.x;
            const ObjTri* otris = tris + id.y;
            HitAcc h{-1, 0.0f, 0.0f, 0.0f};
            bool done = false;
            int otop = 1; st.put(++ptr, 0);
            if (ptr >= kStackCap) { overflow = true; break; }
            while (otop != 0) {
                otop = Objects::step(onodes, otop, o, tm, st, ptr);
                if (ptr >= kStackCap) { overflow = true; break; }
                while (otop < 0) {
                    const int first = ~otop; otop = st.get(ptr); ptr--;
                    if (Objects::template leaf<ANY>(otris, first, o, tm, h)) { done = true; otop = 0; break; }
                }
            }
            if (h.id >= 0) { hit = h; hit_instance = id.z & 0x7FFFFFFF; }
            if (overflow || (ANY && done)) break;
            tmax = o.tmax;
        }
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

template <bool ANY>
__global__ __launch_bounds__(kWave) void k_instanced(const Node2* __restrict__ tlas, const RodentInstance* __restrict__ instances,
                                                     const Node2* __restrict__ nodes, const Tri1* __restrict__ tris,
                                                     const Ray1* __restrict__ rays, Hit1* __restrict__ hits,
                                                     int* __restrict__ hit_instances, int n, Ctl* ctl) {
    __shared__ int stack_lds[kStackCap * kWave];
    instanced_loop<ANY>(tlas, StaticEnter{instances}, nodes, tris, rays, hits, hit_instances, n, ctl, stack_lds);
}

template <bool ANY>
__global__ __launch_bounds__(kWave) void k_instanced_motion(const Node2* __restrict__ tlas,
                                                            const RodentMotionInstance* __restrict__ instances,
                                                            const float* __restrict__ times, const Node2* __restrict__ nodes,
                                                            const Tri1* __restrict__ tris, const Ray1* __restrict__ rays,
                                                            Hit1* __restrict__ hits, int* __restrict__ hit_instances, int n, Ctl* ctl) {
    __shared__ int stack_lds[kStackCap * kWave];
    instanced_loop<ANY>(tlas, MotionEnter{instances, times}, nodes, tris, rays, hits, hit_instances, n, ctl, stack_lds);
}

// Deforming objects under moving instances: the motion TLAS over motion objects, one time per ray through both levels.
template <bool ANY>
__global__ __launch_bounds__(kWave) void k_instanced_motion_objects(const Node2* __restrict__ tlas,
                                                                    const RodentMotionInstance* __restrict__ instances,
                                                                    const float* __restrict__ times,
                                                                    const RodentMotionNode2* __restrict__ nodes,
                                                                    const RodentMotionTri1* __restrict__ tris,
                                                                    const Ray1* __restrict__ rays, Hit1* __restrict__ hits,
                                                                    int* __restrict__ hit_instances, int n, Ctl* ctl) {
    __shared__ int stack_lds[kStackCap * kWave];
    instanced_loop<ANY>(tlas, MotionEnter{instances, times}, nodes, tris, rays, hits, hit_instances, n, ctl, stack_lds,
                        MotionObjects{times});
}
