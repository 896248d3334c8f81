// build_tlas.h -- the top level of an instanced scene (include/rodent_instances.h; included by bvh_build.hip after build_lbvh.h): the
// instance stage (k_instances; k_motion_instances<ObjNode> for moving instances, over static or motion objects) in front of the LBVH's stages 2, 3, 5, 6 and 7 and the leaf stage
// in the place of stage 4.  CPU models: tests/instance_model.py, tests/motion_instance_model.py, tests/motion_objects_model.py.
#pragma once
// invert_affine, the one inverse of the build stage and of k_instanced_motion: instance_inverse.h.

// The widened world box (lo_x hi_x lo_y hi_y lo_z hi_z) of the object box olo / ohi under `m`.
__device__ __forceinline__ void instance_world_box(const float m[12], const float olo[3], const float ohi[3], float box[6]) {
    const float X = fmaxf(fabsf(olo[0]), fabsf(ohi[0])), Y = fmaxf(fabsf(olo[1]), fabsf(ohi[1])), Z = fmaxf(fabsf(olo[2]), fabsf(ohi[2]));
    for (int a = 0; a < 3; a++) {
        const float* r = m + 4 * a;
        float mn = INFINITY, mx = -INFINITY;
        for (int corner = 0; corner < 8; corner++) {
            const float x = (corner & 1) ? ohi[0] : olo[0], y = (corner & 2) ? ohi[1] : olo[1], z = (corner & 4) ? ohi[2] : olo[2];
            const float v = ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
            mn = fminf(mn, v); mx = fmaxf(mx, v);
        }
        const float e = 0x1p-21f * (((fabsf(r[0]) * X + fabsf(r[1]) * Y) + fabsf(r[2]) * Z) + fabsf(r[3]));
        box[2 * a] = canon(mn) - e; box[2 * a + 1] = canon(mx) + e;
    }
}

// ---- the instance stage: inverse, world box, sort point, flags (in the place of k_centroids) ------------------------------------------
// staged[t]: the RodentInstance record of descriptor t without its end-of-leaf bit; wbox[6 t]: its world box; cent[t]: its sort point.
__global__ __launch_bounds__(kBlock) void k_instances(const Node2* __restrict__ nodes, const RodentObject* __restrict__ objects,
                                                      int num_objects, const RodentInstanceDesc* __restrict__ descs, int n,
                                                      RodentInstance* __restrict__ staged, float* __restrict__ wbox,
                                                      float4* __restrict__ cent, float* __restrict__ partial, int* info) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        const float4* dp = reinterpret_cast<const float4*>(descs + t);
        const float4 r0 = dp[0], r1 = dp[1], r2 = dp[2];
        const int4 id = *reinterpret_cast<const int4*>(dp + 3);          // object, instance_id, pad, pad
        const float m[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        int flags = 0, object = id.x;
        if ((unsigned)object >= (unsigned)num_objects) { flags |= RODENT_TLAS_BAD_OBJECT; object = 0; }
        const int4 ob = reinterpret_cast<const int4*>(objects)[object];  // node_offset, tri_offset, num_nodes, num_tris
        float w[12];
        flags |= invert_affine(m, w);
        const float4* np = reinterpret_cast<const float4*>(nodes + ob.x);
        const float4 b0 = np[0], b1 = np[1], b2 = np[2];                 // child 0: b0.x .. b1.y, child 1: b1.z .. b2.w
        const float olo[3] = {fminf(b0.x, b1.z), fminf(b0.z, b2.x), fminf(b1.x, b2.z)};
        const float ohi[3] = {fmaxf(b0.y, b1.w), fmaxf(b0.w, b2.y), fmaxf(b1.y, b2.w)};
        float box[6];
        instance_world_box(m, olo, ohi, box);
        const float s[3] = {box[0] + box[1], box[2] + box[3], box[4] + box[5]};
        float4* out = reinterpret_cast<float4*>(staged + t);
        out[0] = make_float4(w[0], w[1], w[2], w[3]);
        out[1] = make_float4(w[4], w[5], w[6], w[7]);
        out[2] = make_float4(w[8], w[9], w[10], w[11]);
        out[3] = make_float4(__int_as_float(ob.x), __int_as_float(ob.y), __int_as_float(id.y & 0x7FFFFFFF), 0.0f);
        for (int k = 0; k < 6; k++) wbox[6 * (size_t)t + k] = box[k];
        cent[t] = make_float4(s[0], s[1], s[2], 0.0f);
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], s[a]); hi[a] = fmaxf(hi[a], s[a]); }
        if (flags) atomicOr(&info[kInfoFlags], flags);
    }
    block_bounds(lo, hi, partial + 6 * blockIdx.x);
}

// ---- the motion instance stage (in the place of k_instances): both matrices checked, the motion box, its sort point ------------------
// The per-axis widening e of instance_world_box under `m`, restated: the motion box is widened by both endpoints'.
__device__ __forceinline__ void instance_widening(const float m[12], const float olo[3], const float ohi[3], float e[3]) {
    const float X = fmaxf(fabsf(olo[0]), fabsf(ohi[0])), Y = fmaxf(fabsf(olo[1]), fabsf(ohi[1])), Z = fmaxf(fabsf(olo[2]), fabsf(ohi[2]));
    for (int a = 0; a < 3; a++) {
        const float* r = m + 4 * a;
        e[a] = 0x1p-21f * (((fabsf(r[0]) * X + fabsf(r[1]) * Y) + fabsf(r[2]) * Z) + fabsf(r[3]));
    }
}

// The object box from an object's root record: the union of its two child boxes (an empty slot's (+inf, -inf) drops out) -- of a
// two-key root the union over both keys too, the four stored child boxes (rodent_instances.h, "deforming objects under moving
// instances": why it is the union and not key 0's box under M0 and key 1's under M1).
struct ObjectBox { float lo[3], hi[3]; };
__device__ __forceinline__ ObjectBox object_box(const Node2* root) {
    const float4* np = reinterpret_cast<const float4*>(root);
    const float4 b0 = np[0], b1 = np[1], b2 = np[2];                     // child 0: b0.x .. b1.y, child 1: b1.z .. b2.w
    return {{fminf(b0.x, b1.z), fminf(b0.z, b2.x), fminf(b1.x, b2.z)}, {fmaxf(b0.y, b1.w), fmaxf(b0.w, b2.y), fmaxf(b1.y, b2.w)}};
}
__device__ __forceinline__ ObjectBox object_box(const RodentMotionNode2* root) {
    const float4* np = reinterpret_cast<const float4*>(root);
    const float4 b0 = np[0], b1 = np[1], b2 = np[2], c0 = np[3], c1 = np[4], c2 = np[5];     // key 0's rows, key 1's rows
    return {{fminf(fminf(b0.x, b1.z), fminf(c0.x, c1.z)), fminf(fminf(b0.z, b2.x), fminf(c0.z, c2.x)),
             fminf(fminf(b1.x, b2.z), fminf(c1.x, c2.z))},
            {fmaxf(fmaxf(b0.y, b1.w), fmaxf(c0.y, c1.w)), fmaxf(fmaxf(b0.w, b2.y), fmaxf(c0.w, c2.y)),
             fmaxf(fmaxf(b1.y, b2.w), fmaxf(c1.y, c2.w))}};
}

// staged[t]: the RodentMotionInstance record of descriptor t without its end-of-leaf bit; wbox[6 t]: its motion box; cent[t]: its sort
// point.  Stated once over the objects' record type, which decides only how the root is read (object_box).
template <class ObjNode>
__global__ __launch_bounds__(kBlock) void k_motion_instances(const ObjNode* __restrict__ nodes, const RodentObject* __restrict__ objects,
                                                             int num_objects, const RodentMotionInstanceDesc* __restrict__ descs, int n,
                                                             RodentMotionInstance* __restrict__ staged, float* __restrict__ wbox,
                                                             float4* __restrict__ cent, float* __restrict__ partial, int* info) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        const float4* dp = reinterpret_cast<const float4*>(descs + t);
        float4 r[6];
        for (int k = 0; k < 6; k++) r[k] = dp[k];
        const int4 id = *reinterpret_cast<const int4*>(dp + 6);          // object, instance_id, pad, pad
        const float m0[12] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w};
        const float m1[12] = {r[3].x, r[3].y, r[3].z, r[3].w, r[4].x, r[4].y, r[4].z, r[4].w, r[5].x, r[5].y, r[5].z, r[5].w};
        int flags = 0, object = id.x;
        if ((unsigned)object >= (unsigned)num_objects) { flags |= RODENT_TLAS_BAD_OBJECT; object = 0; }
        const int4 ob = reinterpret_cast<const int4*>(objects)[object];  // node_offset, tri_offset, num_nodes, num_tris
        float w[12];                                                     // only the verdicts are kept: the kernel inverts per ray
        flags |= invert_affine(m0, w);
        flags |= invert_affine(m1, w);
        const ObjectBox ub = object_box(nodes + ob.x);
        const float olo[3] = {ub.lo[0], ub.lo[1], ub.lo[2]};
        const float ohi[3] = {ub.hi[0], ub.hi[1], ub.hi[2]};
        float box0[6], box1[6], e0[3], e1[3], box[6];
        instance_world_box(m0, olo, ohi, box0); instance_widening(m0, olo, ohi, e0);
        instance_world_box(m1, olo, ohi, box1); instance_widening(m1, olo, ohi, e1);
        for (int a = 0; a < 3; a++) {
            const float e = e0[a] + e1[a];
            box[2 * a] = fminf(box0[2 * a], box1[2 * a]) - e;
            box[2 * a + 1] = fmaxf(box0[2 * a + 1], box1[2 * a + 1]) + e;
        }
        const float s[3] = {box[0] + box[1], box[2] + box[3], box[4] + box[5]};
        float4* out = reinterpret_cast<float4*>(staged + t);
        for (int k = 0; k < 6; k++) out[k] = r[k];
        out[6] = make_float4(__int_as_float(ob.x), __int_as_float(ob.y), __int_as_float(id.y & 0x7FFFFFFF), 0.0f);
        out[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = 0; k < 6; k++) wbox[6 * (size_t)t + k] = box[k];
        cent[t] = make_float4(s[0], s[1], s[2], 0.0f);
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], s[a]); hi[a] = fmaxf(hi[a], s[a]); }
        if (flags) atomicOr(&info[kInfoFlags], flags);
    }
    block_bounds(lo, hi, partial + 6 * blockIdx.x);
}


// ---- the leaf stage: RodentInstance / RodentMotionInstance records and leaf boxes in sorted order (in the place of k_leaves) ---------
template <class Rec>
__global__ __launch_bounds__(kBlock) void k_tlas_leaves(const Rec* __restrict__ staged, const float* __restrict__ wbox,
                                                        const uint32_t* __restrict__ order, int n,
                                                        Rec* __restrict__ instances, float* __restrict__ leafbox) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const size_t r = order[p];
    const float4* in = reinterpret_cast<const float4*>(staged + r);
    float4* out = reinterpret_cast<float4*>(instances + p);
    for (int k = 0; k < (int)(sizeof(Rec) / 16); k++) out[k] = in[k];
    for (int k = 0; k < 6; k++) leafbox[6 * (size_t)p + k] = wbox[6 * r + k];
}
