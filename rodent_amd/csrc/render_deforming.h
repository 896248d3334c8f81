// render_deforming.h -- deforming meshes in the renderer (include/rodent_render.h, "deforming meshes in the renderer"; included by
// render.hip after render_motion.h): the stream traversal kernels over two-key records with a time per ray.  The shader's deforming form
// is k_shade<.., false, DeformingDev> (render_shade.h), the generation's k_generate<true> (render.hip).  CPU model:
// tests/deforming_scene_model.py.
#pragma once

// k_trace_deforming<false>: the closest-hit pass over a PrimaryStream; <true>: the shadow pass over a SecondaryStream.  The loop is
// k_bvh2_motion's (traversal_motion.h), statement for statement, from the same functions (traversal_motion_steps.h: motion_node2_step,
// leaf_motion_tri1; InstanceStack): one ray per lane, one 64-ray chunk per one-wave workgroup, the whole stack of 64 entries in 16 KB of
// LDS, s = 1 - t taken once per ray.  The time comes as in StreamMotionEnter (render_motion.h): from the depth word's 23 time bits by the
// shutter rule in the closest-hit pass, as float bits from SecondaryStream::prim_id in the shadow pass, loaded behind the same opaque
// copy of the index as the ray.  rodent_motion.h's time rule holds (the stage-level entries let a caller write any word there, and no
// NaN bound may reach the slab test): a closest-hit ray with !(0 <= t && t <= 1) stores the miss record with tmax as given, a shadow
// ray outside is not occluded and adds its colour; such a lane sits out the loop beside its traced neighbours.
// Around the loop the stream I/O of trace_instanced_pass (render_instanced.h) without the slot array: the hit record (the accepted
// triangle's key-0 geom_id and prim_id, or the miss record with tmax bit for bit) through store_hit_record, the primary counter and the
// striped shadow counters, film_add_wave for the shadow rays nothing occludes.  A stack overflow raises *err (the flag frame_end reads)
// and the ray stops where it stands: there is no deep list and no follow-up kernel, so block 0 of the closest-hit pass does that
// kernel's housekeeping for the loop: it zeroes the shader's slot counter.
template <bool ANY>
__global__ __launch_bounds__(kWave) void k_trace_deforming(SceneDev sc, DeformingDev in, PrimaryStream p, SecondaryStream s,
                                                           const int* size_ptr, int n_value, float* film, float inv_spp,
                                                           unsigned long long* counters, int* err, int* zero_word) {
    __shared__ int stack_lds[kStackCap * kWave];
    const int lane = threadIdx.x, chunk = blockIdx.x, i = chunk * kWave + lane;
    // (the grid covers n_value rays: a shadow pass's size may live on the device)
    const int n = ANY ? stream_size(size_ptr, n_value) : n_value;
    if (!ANY && chunk == 0 && lane == 0) { atomicAdd(&counters[0], (unsigned long long)n); *zero_word = 0; }
    if (chunk * kWave >= n) return;
    const RayStream& rays = ANY ? s.rays : p.rays;
    bool active = i < n;
    int pixel = -1;
    if (ANY) {
        pixel = active ? rays.id[i] : -1;
        const unsigned long long live = __ballot(pixel >= 0);
        if (lane == 0 && live) atomicAdd(&counters[4 + (chunk & 63)], (unsigned long long)__popcll(live));
        active = pixel >= 0;
    }
    bool lit = false;
    if (active) {
        InstanceStack st{(lds_int*)stack_lds + lane};
        int k = i;
        asm volatile("" : "+v"(k));
        RayX ray = load_stream_ray(rays, k);
        const int32_t word = (ANY ? s.prim_id : p.depth)[k];
        const float t = ANY ? __int_as_float(word) : shutter_time((uint32_t)word >> RODENT_MOTION_DEPTH_BITS, in.open, in.close);
        HitAccGeom hit; hit.id = -1; hit.t = ray.tmax; hit.u = 0.0f; hit.v = 0.0f; hit.geom = sc.num_materials;
        bool overflow = false, occluded = false;
        if (0.0f <= t && t <= 1.0f) {                                       // the time rule (a NaN fails both comparisons)
            const float s_ = __fsub_rn(1.0f, t);
            int ptr = 0, top = 1; st.put(0, 0);
            while (top != 0) {
                top = motion_node2_step(in.nodes, top, ray, s_, t, st, ptr);
                if (ptr >= kStackCap) { overflow = true; break; }           // the 64th push was not stored: stop where it stands
                while (top < 0) {
                    const int first = ~top; top = st.get(ptr); ptr--;
                    if (leaf_motion_tri1<ANY>(in.tris, first, ray, s_, t, hit)) { occluded = true; top = 0; break; }
                }
            }
        }
        if (overflow) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ANY) lit = !occluded && !overflow;
        else store_hit_record(p, (unsigned)i, hit.geom, hit.id, hit.t, hit.u, hit.v);
    }
    if (ANY) film_add_wave(film, pixel, lit, lit ? s.color_r[i] * inv_spp : 0.0f, lit ? s.color_g[i] * inv_spp : 0.0f,
        lit ? s.color_b[i] * inv_spp : 0.0f);
}
