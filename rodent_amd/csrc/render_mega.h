// render_mega.h -- the renderer's persistent-threads megakernels (K8): k_mega and its joint form k_mega_joint.
//
// Included by render.hip inside its anonymous namespace (after render_trace.h and render_shade.h: trace_one / trace_two, shade_vertex;
// emit_sample is render.hip's).
#pragma once

// ---------------------------------------------------------------------------------------------
// K8: persistent-threads megakernel (mapping_gpu.impala:371-474): one 64-lane workgroup per film tile
// of ~1024 samples; every lane carries a whole path in registers (traverse, shade, shadow-traverse,
// bounce) and fetches the next (pixel, sample) of the tile when its path ends; the path's colour is
// summed locally and added to the film once (:405-407,442,469).  The workgroup is one wavefront, so
// the reference's LDS work counter (:389-395,410) is a wave-uniform register here and the hand-out is
// a ballot prefix: lane order = sample order, deterministic.
// ---------------------------------------------------------------------------------------------
// CURSOR (what ships; round 3): both traversal loops run on the LDS-only cursor stack of the stream kernels (no depth test in the hot
// loop); a ray that outgrows the 15-entry window is traced again with the 64-entry LDS + scratch stack.  +2 % on config 4 and on the
// atrium against the depth-tested stack (3 216 -> 3 276, 586 -> 599 Msamples/s).
template <bool CURSOR>
__global__ __launch_bounds__(kWave) void k_mega(SceneDev sc, CameraDev cam, float* film, int film_w, int film_h, int y0, int y1, int iter,
    int spp,
                                                int max_path_len, int log2_tile, float inv_spp, int* err, unsigned long long* counters) {
    __shared__ int lds[kLdsStack * kWave];
    const int tile = 1 << log2_tile;
    const int tile_x = blockIdx.x * tile, tile_y = y0 + blockIdx.y * tile;
    const int tile_w = min(film_w - tile_x, tile), tile_h = min(y1 - tile_y, tile);
    const int ray_count = tile_w * tile_h * spp;
    StreamStack st; st.col = (lds_int*)lds + threadIdx.x; st.err = err;
    int next = 0;                                   // wave-uniform
    bool has_path = false;
    PathVertex pv; pv.pixel = -1; pv.org = V(0, 0, 0); pv.dir = V(0, 0, 1); pv.rnd = 0; pv.mis = 0.0f; pv.contrib = V(0, 0, 0);
    pv.depth = 0;
    float tmin = 0.0f;
    v3 final_color = V(0, 0, 0);
    unsigned n_primary = 0, n_shadow = 0;
    for (;;) {
        const unsigned long long need = __ballot(!has_path);
        if (need && next < ray_count) {
            const int id = next + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
            next += __popcll(need);
            if (!has_path && id < ray_count) {
                const int ray_id = id / spp, sample = id - ray_id * spp;
                const int in_y = ray_id / tile_w, in_x = ray_id - in_y * tile_w;
                const int x = tile_x + in_x, y = tile_y + in_y;
                pv.dir = emit_sample(cam, iter, film_w, film_h, x, y, sample, &pv.rnd);
                pv.org = LD3(cam.eye);
                pv.pixel = y * film_w + x; pv.mis = 0.0f; pv.contrib = V(1, 1, 1); pv.depth = 0;
                tmin = 0.0f; final_color = V(0, 0, 0);
                has_path = true;
            }
        }
        if (!__ballot(has_path)) break;

        bool done = false;
        ShadeOut o; o.shadow = false; o.s_org = V(0, 0, 0); o.s_dir = V(0, 0, 1); o.s_color = V(0, 0, 0);
        if (has_path) {
            n_primary++;
            const auto on_hit = [&](int prim, int geom, float t, float u, float v) { pv.prim = prim; pv.geom = geom; pv.t = t; pv.u = u;
                pv.v = v; };
            const RayX path_ray = make_rayx(pv.org.x, pv.org.y, pv.org.z, pv.dir.x, pv.dir.y, pv.dir.z, tmin, FLT_MAX_REF);
            bool hit_any;
            if (CURSOR) {
                CursorStack cs; cs.init(st.col, kLdsStack - 1);
                hit_any = trace_one<false>(sc.nodes, sc.tris, path_ray, cs, on_hit);
                // (from the root again: the closest hit is found again)
                if (cs.overflow) hit_any = trace_one<false>(sc.nodes, sc.tris, path_ray, st, on_hit);
            } else hit_any = trace_one<false>(sc.nodes, sc.tris, path_ray, st, on_hit);
            if (!hit_any) done = true;
            else {
                o = shade_vertex(sc, pv, max_path_len);
                if (o.emits) final_color = add(final_color, o.emitted);
                if (o.bounce) { pv.org = o.b_org; pv.dir = o.b_dir; pv.rnd = o.rnd; pv.mis = o.mis; pv.contrib = o.contrib; pv.depth++;
                    tmin = kRayOffset; }
                else done = true;
            }
        }
        if (o.shadow) {
            n_shadow++;
            const RayX shadow_ray = make_rayx(o.s_org.x, o.s_org.y, o.s_org.z, o.s_dir.x, o.s_dir.y, o.s_dir.z, kRayOffset,
                1.0f - kRayOffset);
            const auto nothing = [](int, int, float, float, float) {};
            bool lit;
            if (CURSOR) {
                CursorStack cs; cs.init(st.col, kLdsStack - 1);
                lit = !trace_one<true>(sc.nodes, sc.tris, shadow_ray, cs, nothing);
                if (cs.overflow) lit = !trace_one<true>(sc.nodes, sc.tris, shadow_ray, st, nothing);
            } else lit = !trace_one<true>(sc.nodes, sc.tris, shadow_ray, st, nothing);
            if (lit) final_color = add(final_color, o.s_color);
        }
        film_add_wave(film, pv.pixel, done, final_color.x * inv_spp, final_color.y * inv_spp, final_color.z * inv_spp);
        if (done) has_path = false;
    }
    for (int off = 32; off > 0; off >>= 1) { n_primary += __shfl_xor(n_primary, off); n_shadow += __shfl_xor(n_shadow, off); }
    if (threadIdx.x == 0) {
        const int stripe = (blockIdx.y * gridDim.x + blockIdx.x) & 31;
        atomicAdd(&counters[68 + stripe], (unsigned long long)n_primary);
        atomicAdd(&counters[4 + stripe], (unsigned long long)n_shadow);
    }
}

// Joint form of the megakernel (rodent_hip_render_mega_joint(dev, 1); measured, NOT the default): the shadow ray of a path vertex and
// the path's NEXT ray are traced back to back in one wave-level loop (trace_two) instead of in two loops that each wait for
// their slowest lane; the shader runs between two such loops.  k_mega is issue-bound at 41 % lane utilisation
// (profiles/r03_mega_pmc.txt), and the joint loop does save wave iterations inside a loop -- but a path whose last vertex still
// has a shadow ray pending keeps its lane for one more loop in which it has no path ray to trace, and the phase switch builds
// a second ray (three divisions) inside the loop: config 4 3 225 -> 2 786 Msamples/s, atrium 586 -> 550
// (profiles/r03_render_rates_mega_joint.txt).  Per path the sequence is unchanged (ray, shade, shadow ray, next ray, ...); the
// path's colour is added to the film when both its last ray and its last shadow ray are done.
__global__ __launch_bounds__(kWave) void k_mega_joint(SceneDev sc, CameraDev cam, float* film, int film_w, int film_h, int y0, int y1,
    int iter, int spp,
                                                      int max_path_len, int log2_tile, float inv_spp, int* err,
                                                          unsigned long long* counters) {
    __shared__ int lds[kLdsStack * kWave];
    const int tile = 1 << log2_tile;
    const int tile_x = blockIdx.x * tile, tile_y = y0 + blockIdx.y * tile;
    const int tile_w = min(film_w - tile_x, tile), tile_h = min(y1 - tile_y, tile);
    const int ray_count = tile_w * tile_h * spp;
    StreamStack st; st.col = (lds_int*)lds + threadIdx.x; st.err = err;
    int next = 0;                                   // wave-uniform
    bool has_path = false, has_shadow = false, unpaid = false;      // unpaid: the path's colour has not gone to the film yet
    PathVertex pv; pv.pixel = -1; pv.org = V(0, 0, 0); pv.dir = V(0, 0, 1); pv.rnd = 0; pv.mis = 0.0f; pv.contrib = V(0, 0, 0);
    pv.depth = 0;
    float tmin = 0.0f;
    v3 final_color = V(0, 0, 0), s_dir = V(0, 0, 1), s_color = V(0, 0, 0);
    unsigned n_primary = 0, n_shadow = 0;
    for (;;) {
        const unsigned long long need = __ballot(!has_path && !has_shadow);
        if (need && next < ray_count) {
            const int id = next + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
            next += __popcll(need);
            if (!has_path && !has_shadow && id < ray_count) {
                const int ray_id = id / spp, sample = id - ray_id * spp;
                const int in_y = ray_id / tile_w, in_x = ray_id - in_y * tile_w;
                const int x = tile_x + in_x, y = tile_y + in_y;
                pv.dir = emit_sample(cam, iter, film_w, film_h, x, y, sample, &pv.rnd);
                pv.org = LD3(cam.eye);
                pv.pixel = y * film_w + x; pv.mis = 0.0f; pv.contrib = V(1, 1, 1); pv.depth = 0;
                tmin = 0.0f; final_color = V(0, 0, 0);
                has_path = true; unpaid = true;
            }
        }
        if (!__ballot(has_path || has_shadow)) break;

        n_primary += has_path ? 1u : 0u; n_shadow += has_shadow ? 1u : 0u;
        const TwoHits hits = trace_two(sc.nodes, sc.tris, has_shadow, has_path, pv.org.x, pv.org.y, pv.org.z, s_dir.x, s_dir.y, s_dir.z,
            kRayOffset, 1.0f - kRayOffset,
                                       pv.dir.x, pv.dir.y, pv.dir.z, tmin, FLT_MAX_REF, st,
                                       [&](int prim, int geom, float t, float u, float v) { pv.prim = prim; pv.geom = geom; pv.t = t;
                                           pv.u = u; pv.v = v; });
        if (has_shadow && !hits.a_occluded) final_color = add(final_color, s_color);
        has_shadow = false;
        if (has_path) {
            if (!hits.b_hit) has_path = false;
            else {
                const ShadeOut o = shade_vertex(sc, pv, max_path_len);
                if (o.emits) final_color = add(final_color, o.emitted);
                if (o.shadow) { has_shadow = true; s_dir = o.s_dir; s_color = o.s_color; pv.org = o.s_org; }
                if (o.bounce) { pv.org = o.b_org; pv.dir = o.b_dir; pv.rnd = o.rnd; pv.mis = o.mis; pv.contrib = o.contrib; pv.depth++;
                    tmin = kRayOffset; }
                else has_path = false;
            }
        }
        const bool pay = unpaid && !has_path && !has_shadow;
        film_add_wave(film, pv.pixel, pay, final_color.x * inv_spp, final_color.y * inv_spp, final_color.z * inv_spp);
        if (pay) unpaid = false;
    }
    for (int off = 32; off > 0; off >>= 1) { n_primary += __shfl_xor(n_primary, off); n_shadow += __shfl_xor(n_shadow, off); }
    if (threadIdx.x == 0) {
        const int stripe = (blockIdx.y * gridDim.x + blockIdx.x) & 31;
        atomicAdd(&counters[68 + stripe], (unsigned long long)n_primary);
        atomicAdd(&counters[4 + stripe], (unsigned long long)n_shadow);
    }
}
