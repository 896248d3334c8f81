// render_shade.h -- the renderer's shading stage (K5): one path vertex (shade_vertex), the look-back scan of the fused compaction and
// k_shade.
//
// Included by render.hip inside its anonymous namespace (after render_trace.h: film_add_wave, the hit-record accessors).
#pragma once

// ---------------------------------------------------------------------------------------------
// K5: shading (mapping_gpu.impala:82-134; renderer.impala:69-152).  One launch over the sorted,
// hit-only prefix of the stream; the material is a table entry, not generated code.
// ---------------------------------------------------------------------------------------------
// One path vertex in registers: what a primary-stream entry holds (driver.impala:63-104).
struct PathVertex {
    int pixel; v3 org, dir; int prim, geom; float t, u, v;
    uint32_t rnd; float mis; v3 contrib; int depth;
};
// What shading a vertex produces: an emission sample, at most one shadow ray, at most one continuation.
struct ShadeOut {
    bool emits; v3 emitted;
    bool shadow; v3 s_org, s_dir, s_color;
    bool bounce; v3 b_org, b_dir, contrib; uint32_t rnd; float mis;
};
constexpr float kRayOffset = 0.001f;           // renderer.impala:46

// RODENT_SHADE_HOIST_LIGHT (compile time): 0 = the light record is fetched where it is used, behind the material (until
// round 5); 1 = fetched into registers in front of the hit's gathers; 2 = its two cache lines touched from k_shade (global_load ... lds
// into a sink row: no register) as soon as the path's random state is in (what ships: k_shade 916 -> 851 us per call at 16 spp, frames +0.2
// %; mode 1 spills ten VGPRs and is 11 % slower).  profiles/r06_shade_*.txt
#ifndef RODENT_SHADE_HOIST_LIGHT
#define RODENT_SHADE_HOIST_LIGHT 2
#endif
// INST (instanced scenes, k_shade<.., true>): pv.prim indexes the concatenated tables and `frame` is the instance the hit lies in -- the
// surface frame goes through its world_to_object rows (surface_element_instanced) and the emitter of a hit is a WORLD light, frame->
// light_offset behind the object's own id; next-event estimation samples sc.lights, which are the world lights then.  Nothing else differs.
template <bool INST> __device__ __forceinline__ Surf hit_surface(const SceneDev& sc, const PathVertex& pv, const InstanceFrame* frame) {
    if constexpr (INST) return surface_element_instanced(&sc, frame, pv.org, pv.dir, pv.prim, pv.t, pv.u, pv.v);
    else return surface_element(&sc, pv.org, pv.dir, pv.prim, pv.t, pv.u, pv.v);
}
// GIVEN (deforming meshes, k_shade<.., false, DeformingDev>): the caller computed the surface (surface_element_deforming) and passes it;
// everything else is the flat shading.
template <bool INST = false, bool GIVEN = false>
__device__ __forceinline__ ShadeOut shade_vertex(const SceneDev& sc, const PathVertex& pv, int max_path_len,
    const InstanceFrame* frame = nullptr, const Surf* given = nullptr) {
    ShadeOut o;
    const float pdf_lightpick = 1.0f / (float)sc.num_lights;
    uint32_t rnd = pv.rnd;
#if RODENT_SHADE_HOIST_LIGHT == 1
    // The light that next-event estimation will sample depends on the path's random state only (renderer.impala:76-78), not on what was
    // hit: its record is fetched HERE, beside the hit's own gathers (material, triangle record), instead of behind them -- one dependent
    // fetch less in the chain this kernel waits for. Same values, same arithmetic; a specular hit fetches a record it
    // does not use.
    typedef float lf4 __attribute__((ext_vector_type(4)));
    lf4 lv0, lv1, lv2, lnrm, lcol;
    {
        uint32_t peek = rnd;
        const RodentLight* Lh = sc.lights + (int)(xorshift(&peek) & 0x7FFFFFFFu) % sc.num_lights;
        lv0 = *reinterpret_cast<const lf4*>(Lh->v0); lv1 = *reinterpret_cast<const lf4*>(Lh->v1);
        lv2 = *reinterpret_cast<const lf4*>(Lh->v2);
        lnrm = *reinterpret_cast<const lf4*>(Lh->n); lcol = *reinterpret_cast<const lf4*>(Lh->color);
    }
#endif
    RodentMaterial textured;
    const RodentMaterial* m = resolve_material(&sc, sc.materials + pv.geom, &textured, pv.prim, pv.u, pv.v);
    const Surf sf = [&] { if constexpr (GIVEN) return *given; else return hit_surface<INST>(sc, pv, frame); }();
    const v3 out_dir = neg(pv.dir);

    // on_hit (renderer.impala:113-128)
    o.emitted = V(0, 0, 0);
    o.emits = m->emissive && sf.entering;
    if (o.emits) {
        const RodentLight* L = sc.lights
            + (INST ? sc.light_ids[pv.prim] + frame->light_offset : sc.light_ids[pv.prim]);
        const float pdf_dir = cosine_hemisphere_pdf(dot(LD3(L->n), out_dir));
        const v3 intensity = pdf_dir > 0.0f ? LD3(L->color) : V(0, 0, 0);
        const float pdf_area = pdf_dir > 0.0f ? L->inv_area : 1.0f;
        const float next_mis = pv.mis * pv.t * pv.t / dot(out_dir, sf.local.c2);
        const float w = 1.0f / (1.0f + next_mis * pdf_lightpick * pdf_area);
        o.emitted = mulf(mulf(mul(pv.contrib, intensity), w), 1.0f);
    }

    // on_shadow (renderer.impala:69-111)
    o.shadow = false;
    if (!bsdf_is_specular(m)) {
        const int light_id = (int)(xorshift(&rnd) & 0x7FFFFFFFu) % sc.num_lights;
        const float lu = randf(&rnd), lv = randf(&rnd);
#if RODENT_SHADE_HOIST_LIGHT == 1
        (void)light_id;
        const v3 pos = sample_triangle(lu, lv, V(lv0.x, lv0.y, lv0.z), V(lv1.x, lv1.y, lv1.z), V(lv2.x, lv2.y, lv2.z));
        const v3 from_dir = sub(sf.point, pos);
        float lcos = dot(from_dir, V(lnrm.x, lnrm.y, lnrm.z)) / len(from_dir);
        v3 intensity = V(lcol.x, lcol.y, lcol.z); float pdf_area = lnrm.w;
#else
        const RodentLight* L = sc.lights + light_id;
        const v3 pos = sample_triangle(lu, lv, LD3(L->v0), LD3(L->v1), LD3(L->v2));
        const v3 from_dir = sub(sf.point, pos);
        float lcos = dot(from_dir, LD3(L->n)) / len(from_dir);
        v3 intensity = LD3(L->color); float pdf_area = L->inv_area;
#endif
        if (!(pdf_area > 0.0f && cosine_hemisphere_pdf(lcos) > 0.0f && lcos > 0.0f)) { intensity = V(0, 0, 0); pdf_area = 1.0f;
            lcos = 0.0f; }
        const v3 light_dir = sub(pos, sf.point);
        const float vis = dot(light_dir, sf.local.c2);
        if (vis > 0.0f && lcos > 0.0f) {
            const float inv_d = 1.0f / len(light_dir), inv_d2 = inv_d * inv_d;
            const v3 in_dir = mulf(light_dir, inv_d);
            const float pdf_e = bsdf_pdf(m, &sf, in_dir, out_dir);
            const float pdf_l = pdf_area * pdf_lightpick, inv_pdf_l = 1.0f / pdf_l;
            const float cos_e = vis * inv_d, cos_l = lcos;
            const float w = 1.0f / (1.0f + pdf_e * cos_l * inv_d2 * inv_pdf_l);
            const float geom = cos_e * cos_l * inv_d2 * inv_pdf_l;
            o.s_color = mulf(mul(intensity, mul(pv.contrib, bsdf_eval(m, &sf, in_dir, out_dir))), geom * w);
            o.s_org = sf.point; o.s_dir = light_dir;
            o.shadow = true;
        }
    }

    // on_bounce (renderer.impala:130-152)
    const float lum2 = 2.0f * luminance(pv.contrib); const float rr = lum2 > 0.75f ? 0.75f : lum2;
    o.bounce = false;
    if (pv.depth >= max_path_len || randf(&rnd) >= rr) return o;
    const BsdfSample bs = bsdf_sample(m, &sf, &rnd, out_dir);
    o.contrib = mulf(mul(pv.contrib, bs.color), bs.cos / (bs.pdf * rr));
    o.b_org = sf.point; o.b_dir = bs.in_dir;
    o.rnd = rnd; o.mis = bsdf_is_specular(m) ? 0.0f : 1.0f / bs.pdf;
    o.bounce = true;
    return o;
}

// Block-wide exclusive prefix over all EARLIER blocks of a launch, single pass ("decoupled look-back"): every block publishes
// its own total as soon as it knows it (flag A), then adds up its predecessors' words -- 64 at a time, one per lane -- back to
// the nearest block that already knows its inclusive prefix (flag P), and publishes its own.  A word is (flag << 30) | value;
// the array is zeroed before the launch (flag 0 = nothing yet: wait).  A block never waits for a LATER one, so the chain ends as long as
// every earlier block is resident or finished -- which holds because the hardware dispatches workgroups in index order, but is not
// something HIP promises: the wait is therefore BOUNDED (about a second of polling, then the kernel traps and the host reports a HIP
// error instead of hanging).  This is the opt-in mode rodent_hip_render_fused_compact(dev, 1) (reproducible stream order); the default,
// mode 2, takes one atomic per block and waits for nobody.  The values are all that travels (relaxed agent-scope atomics, no fences).
// Called by the first wave of the block; returns the prefix in every lane.
constexpr unsigned kScanA = 1u << 30, kScanP = 2u << 30, kScanValue = (1u << 30) - 1u;
// k_shade's `scan` argument for "slots from one atomic counter" (rodent_hip_render_fused_compact(dev, 2))
unsigned* const kScanAtomic = reinterpret_cast<unsigned*>(8);
__device__ __forceinline__ unsigned lookback_exclusive(unsigned* status, int block, unsigned total) {
    const int lane = threadIdx.x;                                        // 0..63
    if (lane == 0) __hip_atomic_store(&status[block], (block == 0 ? kScanP : kScanA) | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (block == 0) return 0u;
    unsigned excl = 0u;
    for (int j = block - 1;; j -= kWave) {
        unsigned long long upto, is_p;
        unsigned w;
        int first_p;
        for (unsigned polls = 0;; polls++) {
            if (polls == (1u << 23)) __builtin_trap();                   // a predecessor that never published: see above
            const int idx = j - lane;
            // in front of block 0: prefix 0
            w = idx >= 0 ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kScanP;
            is_p = __ballot((w >> 30) == 2u);
            first_p = is_p ? __ffsll((long long)is_p) - 1 : kWave - 1;
            upto = first_p >= 63 ? ~0ull : ((2ull << first_p) - 1ull);
            if (!(__ballot((w >> 30) == 0u) & upto)) break;              // every word up to the nearest prefix is there
            __builtin_amdgcn_s_sleep(2);
        }
        unsigned v = ((upto >> lane) & 1ull) ? (w & kScanValue) : 0u;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        excl += v;
        if (is_p) break;
    }
    if (lane == 0) __hip_atomic_store(&status[block], kScanP | (excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// `perm` != nullptr: the sort did not move the rays, it only computed where each would go (perm[sorted position] = stream
// index); thread i then shades ray perm[i] of `p`.  `perm` == nullptr: thread i shades ray i.
// `scan` == nullptr (the stage-level hip_shade, mapping_gpu.impala:82-134 as it stands): the ray that goes on is written to
// slot i of `q` (q == p: in place), a path that ends leaves id -1 behind and gpu_compact_primary (:267-300) squeezes the
// stream afterwards.  `scan` != nullptr (the renderer's loop): COMPACTION IS PART OF THE SHADER -- the ray that goes on is
// written straight to its compacted slot of `q` (another stream than `p`): slot = rays that go on in earlier blocks
// (lookback_exclusive over the blocks' totals) + those in earlier waves of the block + those in lower lanes.  That is the
// stable order the separate compaction produced, without reading and writing the 15-word stream once more per bounce (the
// compaction's copy was 38 % of the summed kernel time of BASELINE config 4, profiles/r02_render_pmc_digest.txt); the
// new stream size goes to *alive_total.
// INST = true (launched for instanced scenes only, with ONE trailing InstancedDev argument; k_shade<kBlock, false> takes none and is the
// kernel as it was): ray `src` lies in the instance at leaf-order slot ray_slots[src]; its record gives the world_to_object rows and the
// instance id k, bases[k] the object's first triangle and the offset of its lights (rules: include/rodent_render.h).
// Its register budget is that of 7 waves per SIMD: under the flat shader's 8 the frame's rows cost it two spilled VGPRs.
// A MOVING scene (k_shade<kBlock, true, MotionDev>): the depth word holds depth | ubits << 8 (rodent_render.h); the record at the ray's
// slot is a RodentMotionInstance, t comes from the word by the shutter rule and the frame is invert(lerp(M0, M1, t)) through
// motion_frame, the function the traversal entered the instance with.  The ray that goes on carries (depth + 1) | ubits << 8, the
// shadow ray t's bits in s.prim_id.  Its register budget: kShadeMotionWaves.

// The frame of a motion record at time t: the seven 16-byte loads of traversal_instanced.h's MotionEnter, lerp_affine, invert_affine
// (instance_inverse.h).  The traversal (render_motion.h) and the shader both call THIS, with the same record and the same t, so the
// shader's 12 floats are the traversal's.  Returns false when the inverse refuses the interpolated matrix.
__device__ __forceinline__ bool motion_frame(const RodentMotionInstance* instances, int j, float t, float w[12], int4& id) {
    const float4* p = reinterpret_cast<const float4*>(instances + j);
    float4 r[6];
    for (int k = 0; k < 6; k++) r[k] = p[k];
    id = *reinterpret_cast<const int4*>(p + 6);                         // node_offset, tri_offset, instance_id, pad
    const float m0[12] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w};
    const float m1[12] = {r[3].x, r[3].y, r[3].z, r[3].w, r[4].x, r[4].y, r[4].z, r[4].w, r[5].x, r[5].y, r[5].z, r[5].w};
    float m[12];
    lerp_affine(m0, m1, t, m);
    return invert_affine(m, w) == 0;
}
// A DEFORMING scene (k_shade<kBlock, false, DeformingDev>): the depth word and the shadow ray's prim_id as for a moving scene; the hit is
// shaded on the surface at its own time (surface_element_deforming: twelve gathers through the index row, the two keys' corners and
// corner normals interpolated by the traversal's lerp rule, the face normal from the interpolated corners), the rest is the flat
// shader's: pv.prim indexes the tables directly and the emitter of a hit is sc.lights[light_ids[prim]].  Its register budget:
// kShadeDeformWaves.
#ifndef RODENT_SHADE_MOTION_WAVES
#define RODENT_SHADE_MOTION_WAVES 5      // (compile time) 7: 20 ... 26 spilled VGPRs, 6: 9 ... 13, 5: none beyond the flat shader's 68 bytes
#endif
constexpr int kShadeMotionWaves = RODENT_SHADE_MOTION_WAVES;
template <bool INST, typename... Inst> constexpr bool shade_motion() { return (std::is_same<Inst, MotionDev>::value || ...); }
#ifndef RODENT_SHADE_DEFORM_WAVES
#define RODENT_SHADE_DEFORM_WAVES 5      // (compile time) 8: 34 ... 36 spilled VGPRs, 7: 24 ... 25, 6: 16, 5: none beyond the flat shader's 68 bytes
#endif
constexpr int kShadeDeformWaves = RODENT_SHADE_DEFORM_WAVES;
template <bool INST, typename... Inst> constexpr bool shade_deforming() { return (std::is_same<Inst, DeformingDev>::value || ...); }
template <bool INST, typename... Inst> constexpr int shade_waves() {
    return shade_deforming<INST, Inst...>() ? kShadeDeformWaves : shade_motion<INST, Inst...>() ? kShadeMotionWaves : INST ? 7 : 8;
}
template <int kBlock /* threads per workgroup = rays per compaction slot request (shade_block()) */, bool INST = false, typename... Inst>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(shade_waves<INST, Inst...>(), 8))) void k_shade(SceneDev sc,
    PrimaryStream p,
    PrimaryStream q, const int* __restrict__ perm, SecondaryStream s, const int* size_ptr, int n_value, float* film,
                                                   float inv_spp, int max_path_len, int unsorted, unsigned* scan, int* alive_total,
                                                   Inst... inst) {
    constexpr bool MOTION = shade_motion<INST, Inst...>(), DEFORM = shade_deforming<INST, Inst...>();
    static_assert(sizeof...(Inst) == (INST || DEFORM ? 1 : 0) && !(INST && DEFORM),
                  "k_shade<.., true> takes one InstancedDev or MotionDev, k_shade<.., false> nothing or one DeformingDev");
    int time_bits = 0;                                                  // MOTION, DEFORM: the depth word's bits above the depth
    float time = 0.0f;
    __shared__ unsigned wave_total[kBlock / kWave + 1];
#if RODENT_SHADE_HOIST_LIGHT == 2
    __shared__ int light_sink[kBlock];
#endif
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int n_valid = stream_size(size_ptr, n_value);
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    // whole block (whole wave) beyond the stream
    if (scan ? (int)(blockIdx.x * kBlock) >= n_valid : (int)(blockIdx.x * kBlock + wave * kWave) >= n_valid) return;
    // Every lane of the wave reaches the ONE film_add_wave call below (it reduces across lanes with shuffles, which must
    // not read lanes that took another path): lanes beyond the stream and rays that missed take part with nothing to add.
    const bool in_range = i < n_valid;
    const int src = (perm && in_range) ? perm[i] : i;
    const bool live = in_range && !(unsorted && load_hit_geom(p, (unsigned)src) >= sc.num_materials);
    if (in_range && !live) { if (!scan) q.rays.id[i] = -1; s.rays.id[i] = -1; }            // unsorted stream: a ray that missed ends here
    PathVertex pv; pv.pixel = -1; pv.depth = 0;
    ShadeOut o; o.emits = false; o.shadow = false; o.bounce = false; o.emitted = V(0, 0, 0);
    if (live) {
        pv.pixel = p.rays.id[src];
        pv.org = V(p.rays.org_x[src], p.rays.org_y[src], p.rays.org_z[src]);
        pv.dir = V(p.rays.dir_x[src], p.rays.dir_y[src], p.rays.dir_z[src]);
        const HitRecord hit = load_hit_record(p, (unsigned)src);
        pv.prim = hit.prim; pv.geom = hit.geom; pv.t = hit.t; pv.u = hit.u; pv.v = hit.v;
        pv.rnd = p.rnd[src]; pv.mis = p.mis[src];
#if RODENT_SHADE_HOIST_LIGHT == 2
        {
            uint32_t peek = pv.rnd;
            const char* lp = reinterpret_cast<const char*>(sc.lights + (int)(xorshift(&peek) & 0x7FFFFFFFu) % sc.num_lights);
            __attribute__((address_space(3))) void* sink =
                (__attribute__((address_space(3))) void*)(light_sink + (threadIdx.x / kWave) * kWave);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)lp, sink, 4, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(lp + 64), sink, 4, 0, 0);
        }
#endif
        pv.contrib = V(p.contrib_r[src], p.contrib_g[src], p.contrib_b[src]);
        pv.depth = p.depth[src];
        if constexpr (MOTION) {
            const MotionDev& in = (inst, ...);
            time_bits = pv.depth & ~RODENT_MOTION_DEPTH_MASK; pv.depth &= RODENT_MOTION_DEPTH_MASK;
            time = shutter_time((uint32_t)time_bits >> RODENT_MOTION_DEPTH_BITS, in.open, in.close);
            float w[12];
            int4 id;
            (void)motion_frame(in.instances, in.ray_slots[src], time, w, id);      // (a hit lies in an instance that was not skipped)
            InstanceFrame frame;
            frame.w0 = make_float4(w[0], w[1], w[2], w[3]); frame.w1 = make_float4(w[4], w[5], w[6], w[7]);
            frame.w2 = make_float4(w[8], w[9], w[10], w[11]);
            const int2 base = in.bases[id.z & 0x7FFFFFFF];
            pv.prim += base.x; frame.light_offset = base.y;
            o = shade_vertex<true>(sc, pv, max_path_len, &frame);
        } else if constexpr (DEFORM) {
            const DeformingDev& in = (inst, ...);
            time_bits = pv.depth & ~RODENT_MOTION_DEPTH_MASK; pv.depth &= RODENT_MOTION_DEPTH_MASK;
            time = shutter_time((uint32_t)time_bits >> RODENT_MOTION_DEPTH_BITS, in.open, in.close);
            const Surf sf = surface_element_deforming(&sc, &in, __fsub_rn(1.0f, time), time, pv.org, pv.dir, pv.prim, pv.t, pv.u, pv.v);
            o = shade_vertex<false, true>(sc, pv, max_path_len, nullptr, &sf);
        } else if constexpr (INST) {
            const InstancedDev& in = (inst, ...);
            const float4* rec = reinterpret_cast<const float4*>(in.instances + in.ray_slots[src]);
            InstanceFrame frame;
            frame.w0 = rec[0]; frame.w1 = rec[1]; frame.w2 = rec[2];
            const int2 base = in.bases[reinterpret_cast<const int4*>(rec + 3)->z & 0x7FFFFFFF];
            pv.prim += base.x; frame.light_offset = base.y;
            o = shade_vertex<true>(sc, pv, max_path_len, &frame);
        } else
        o = shade_vertex(sc, pv, max_path_len);
    }
    film_add_wave(film, pv.pixel, live && o.emits, o.emitted.x * inv_spp, o.emitted.y * inv_spp, o.emitted.z * inv_spp);

    // the secondary ray is written at the SAME index (mapping_gpu.impala:111-115)
    if (live) {
        if (o.shadow) {
            s.rays.org_x[i] = o.s_org.x; s.rays.org_y[i] = o.s_org.y; s.rays.org_z[i] = o.s_org.z;
            s.rays.dir_x[i] = o.s_dir.x; s.rays.dir_y[i] = o.s_dir.y; s.rays.dir_z[i] = o.s_dir.z;
            s.rays.tmin[i] = kRayOffset; s.rays.tmax[i] = 1.0f - kRayOffset;
            s.color_r[i] = o.s_color.x; s.color_g[i] = o.s_color.y; s.color_b[i] = o.s_color.z;
            if constexpr (MOTION || DEFORM) s.prim_id[i] = __float_as_int(time);
        }
        s.rays.id[i] = o.shadow ? pv.pixel : -1;
    }

    const bool goes_on = live && o.bounce;
    int d = i;
    if (scan) {
        const unsigned long long on = __ballot(goes_on);
        if (lane == 0) wave_total[wave] = (unsigned)__popcll(on);
        __syncthreads();
        unsigned before = 0u, total = 0u;
        for (int w = 0; w < kBlock / kWave; w++) { const unsigned c = wave_total[w]; if (w < wave) before += c; total += c; }
        if (wave == 0) {
            // experiment: one returning atomic per block (order of the blocks = order of arrival)
            if (scan == kScanAtomic) {
                if (lane == 0) wave_total[kBlock / kWave] = total ? (unsigned)atomicAdd(alive_total, (int)total) : 0u;
            } else {
                const unsigned excl = lookback_exclusive(scan, blockIdx.x, total);
                if (lane == 0) {
                    wave_total[kBlock / kWave] = excl;
                    // the stream's last block: the new size
                    if ((int)blockIdx.x == (n_valid - 1) / kBlock) *alive_total = (int)(excl + total);
                }
            }
        }
        __syncthreads();
        d = (int)(wave_total[kBlock / kWave] + before) + __popcll(on & ((1ull << lane) - 1ull));
    } else if (live && !goes_on) q.rays.id[i] = -1;
    if (!goes_on) return;
    if (perm || scan) q.rays.id[d] = pv.pixel;                                             // (in place the id is there already)
    q.rays.org_x[d] = o.b_org.x; q.rays.org_y[d] = o.b_org.y; q.rays.org_z[d] = o.b_org.z;
    q.rays.dir_x[d] = o.b_dir.x; q.rays.dir_y[d] = o.b_dir.y; q.rays.dir_z[d] = o.b_dir.z;
    q.rays.tmin[d] = kRayOffset; q.rays.tmax[d] = FLT_MAX_REF;
    q.rnd[d] = o.rnd; q.mis[d] = o.mis;
    q.contrib_r[d] = o.contrib.x; q.contrib_g[d] = o.contrib.y; q.contrib_b[d] = o.contrib.z;
    q.depth[d] = MOTION || DEFORM ? (pv.depth + 1) | time_bits : pv.depth + 1;
}
