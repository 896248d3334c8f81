// render_motion.h -- moving instances in the renderer (include/rodent_render.h, "moving instances in the renderer"; included by
// render.hip after render_instanced.h): the stream traversal kernels over the motion TLAS with a time per ray, and the kernels that
// derive a moving scene's tables from its two sets of matrices.  The shader's moving form is k_shade<.., true, MotionDev>
// (render_shade.h), the generation's k_generate<true> (render.hip).  CPU model: tests/motion_scene_model.py.
#pragma once

// The time of stream index i: the closest-hit pass recomputes it from the depth word's 23 time bits by the shutter rule, the shadow pass
// reads it as float bits from SecondaryStream::prim_id.
template <bool ANY> struct StreamMotionEnter {
    const RodentMotionInstance* instances;
    const int32_t* words;                                               // ANY: s.prim_id, else p.depth
    float open, close;
    __device__ __forceinline__ bool enter(int j, int i, const RayX& ray, RayX& o, int4& id) const {
        const int32_t word = words[i];                                  // (i: the opaque copy the ray was loaded behind)
        const float t = ANY ? __int_as_float(word) : shutter_time((uint32_t)word >> RODENT_MOTION_DEPTH_BITS, open, close);
        float w[12];
        if (!motion_frame(instances, j, t, w, id)) return false;       // singular or non-finite at this ray's time: skipped, no flag
        o = object_ray(ray, make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]),
                       make_float4(w[8], w[9], w[10], w[11]));
        return true;
    }
};

// k_trace_instanced's pass (trace_instanced_pass) over motion records: only the record-to-object-ray step differs.
template <bool ANY>
__global__ __launch_bounds__(kWave) void k_trace_instanced_motion(SceneDev sc, MotionDev in, PrimaryStream p, SecondaryStream s,
                                                                  const int* size_ptr, int n_value, float* film, float inv_spp,
                                                                  unsigned long long* counters, int* err, int* zero_word) {
    __shared__ int stack_lds[kStackCap * kWave];
    trace_instanced_pass<ANY>(sc, in.tlas, StreamMotionEnter<ANY>{in.instances, ANY ? s.prim_id : p.depth, in.open, in.close},
                              in.ray_slots, p, s, size_ptr, n_value, film, inv_spp, counters, err, zero_word, stack_lds);
}

// ---- the tables a moving scene derives (rodent_hip_scene_create_motion, rodent_hip_scene_set_motion_transforms) ----------------------
// One thread per matrix entry of either key: the moved matrices into the descriptor array; the object and id words stay.
__global__ __launch_bounds__(kBlock) void k_motion_instance_matrices(const float* __restrict__ m0, const float* __restrict__ m1,
                                                                     int num_instances, RodentMotionInstanceDesc* __restrict__ descs) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 24 * num_instances) return;
    const int k = t / 24, e = t % 24;
    if (e < 12) descs[k].object_to_world0[e] = m0[12 * k + e];
    else descs[k].object_to_world1[e - 12] = m1[12 * k + e - 12];
}

// One thread per leaf-order slot: slot_of[instance id] = slot (k_slot_of over motion records, whose id word lies elsewhere).
__global__ __launch_bounds__(kBlock) void k_motion_slot_of(const RodentMotionInstance* __restrict__ instances, int num_instances,
                                                           int* __restrict__ slot_of) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= num_instances) return;
    const int k = instances[j].instance_id & 0x7FFFFFFF;
    if (k < num_instances) slot_of[k] = j;
}

// One thread per world light: k_world_lights under M0, with w = invert_affine(M0) taken here (a motion record stores no inverse; a
// refused inverse leaves what it computed: the rebuild raised RODENT_TLAS_BAD_TRANSFORM and the tables are undefined anyway).
__global__ __launch_bounds__(kBlock) void k_motion_world_lights(const RodentMotionInstanceDesc* __restrict__ descs,
                                                                const int* __restrict__ light_owner, const int2* __restrict__ bases,
                                                                const RodentLight* __restrict__ object_lights, int num_lights,
                                                                RodentLight* __restrict__ lights) {
    const int l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= num_lights) return;
    const int k = light_owner[l];
    const RodentLight src = object_lights[l - bases[k].y];
    float m[12], w[12];
    for (int e = 0; e < 12; e++) m[e] = descs[k].object_to_world0[e];
    (void)invert_affine(m, w);
    // from here on k_world_lights' statements (stated again: shared through a function, that kernel lost a register of its row)
    RodentLight out = src;                                            // the corners' fourth words and the colour stay
    const float* in_v[3] = {src.v0, src.v1, src.v2};
    float* out_v[3] = {out.v0, out.v1, out.v2};
    for (int c = 0; c < 3; c++)
        for (int a = 0; a < 3; a++) out_v[c][a] = row_point(m + 4 * a, in_v[c][0], in_v[c][1], in_v[c][2]);
    const float ax = __fsub_rn(out.v1[0], out.v0[0]), ay = __fsub_rn(out.v1[1], out.v0[1]), az = __fsub_rn(out.v1[2], out.v0[2]);
    const float bx = __fsub_rn(out.v2[0], out.v0[0]), by = __fsub_rn(out.v2[1], out.v0[1]), bz = __fsub_rn(out.v2[2], out.v0[2]);
    const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by)), cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz)),
        cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
    out.inv_area = __fdiv_rn(1.0f, __fmul_rn(0.5f, sqrtf(length2(cx, cy, cz))));
    float nw[3];
    for (int a = 0; a < 3; a++)
        nw[a] = __fadd_rn(__fadd_rn(__fmul_rn(w[a], src.n[0]), __fmul_rn(w[4 + a], src.n[1])), __fmul_rn(w[8 + a], src.n[2]));
    const float inv = __fdiv_rn(1.0f, sqrtf(length2(nw[0], nw[1], nw[2])));
    for (int a = 0; a < 3; a++) out.n[a] = __fmul_rn(nw[a], inv);
    lights[l] = out;
}
