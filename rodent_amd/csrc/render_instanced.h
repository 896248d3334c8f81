// render_instanced.h -- instanced scenes in the renderer (include/rodent_render.h, "instanced scenes"; included by render.hip after
// render_update.h): the stream traversal kernels over the two-level hierarchy and the kernels that derive the scene's tables from the
// instances' matrices, and the kernels that rederive the tables of deforming objects.  CPU models: tests/instanced_scene_model.py,
// tests/instanced_deform_model.py.
#pragma once

// k_trace_instanced<false>: the closest-hit pass over a PrimaryStream; <true>: the shadow pass over a SecondaryStream.  The loop is
// k_instanced's (traversal_instanced.h), statement for statement, from the same functions (traversal_steps.h: node2_step, leaf_tri1,
// object_ray, InstanceStack): one ray per lane, one 64-ray chunk per one-wave workgroup, ONE loop whose iteration is either a TLAS step or
// a whole instance, the world ray reloaded from the stream behind an opaque copy of the index (nested, the compiler kept the ray's slab
// operands in scratch: DESIGN 11), one stack of 64 entries in 16 KB of LDS for both levels.  Around it the stream I/O of k_trace_primary /
// k_trace_secondary: the hit record (the accepted Tri1's geom_id and its OBJECT-LOCAL prim_id, or the miss record with tmax bit for bit)
// through store_hit_record, the instance's leaf-order slot (-1 on a miss) into ray_slots, the primary counter and the striped shadow
// counters, film_add_wave for the shadow rays nothing occludes.  A stack overflow raises *err (the flag frame_end reads) and the ray
// stops where it stands: there is no deep list and no follow-up kernel, so block 0 of the closest-hit pass does that kernel's
// housekeeping for the loop: it zeroes the shader's slot counter.  (The ticket counters are the persistent kernels', which an instanced
// scene never launches: they stay zero.)  The pass is stated once, trace_instanced_pass, for this kernel and k_trace_instanced_motion
// (render_motion.h); they differ in how a record yields the object ray.

// How an instance record yields the object ray, as in traversal_instanced.h: enter(j, i, ray, o, id) reads record j for stream index i
// (the opaque copy), fills the object ray and id = {node_offset, tri_offset, instance_id, pad}, and returns whether the instance is
// entered at all.  The static form; the moving one is StreamMotionEnter (render_motion.h).
struct StreamStaticEnter {
    const RodentInstance* instances;
    __device__ __forceinline__ bool enter(int j, int, const RayX& ray, RayX& o, int4& id) const {
        const float4* rec = reinterpret_cast<const float4*>(instances + j);
        const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
        id = *reinterpret_cast<const int4*>(rec + 3);                   // node_offset, tri_offset, instance_id, pad
        o = object_ray(ray, w0, w1, w2);
        return true;
    }
};

// The pass of both kernels (k_trace_instanced, k_trace_instanced_motion), stated once.
template <bool ANY, class Enter>
__device__ __forceinline__ void trace_instanced_pass(const SceneDev& sc, const Node2* __restrict__ tlas, const Enter& in,
                                                     int32_t* ray_slots, const PrimaryStream& p, const SecondaryStream& s,
                                                     const int* size_ptr, int n_value, float* film, float inv_spp,
                                                     unsigned long long* counters, int* err, int* zero_word, int* stack_lds) {
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
        const float tmax_given = rays.tmax[i];
        float tmax = tmax_given;
        HitAccGeom hit; hit.id = -1; hit.t = tmax_given; hit.u = 0.0f; hit.v = 0.0f; hit.geom = sc.num_materials;
        int slot = -1;
        int ptr = 0, top = 1; st.put(0, 0);
        int j = -1;                                                         // the instance to enter next, -1: a TLAS step is next
        bool overflow = false, occluded = false;
        while (top != 0) {
            int again = i;
            asm volatile("" : "+v"(again));
            RayX ray = load_stream_ray(rays, again);
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
                const Node2* onodes = sc.nodes + id.x;
                const Tri1* otris = sc.tris + id.y;
                HitAccGeom h; h.id = -1; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.geom = 0;
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
                if (h.id >= 0) { hit = h; slot = j; }
                if (ANY && done) occluded = true;
                if (overflow || (ANY && done)) break;
                tmax = o.tmax;
            }
            j++;
            if (id.z < 0) {                                                 // the last instance of the leaf: on with its continuation
                top = st.get(ptr); ptr--;
                j = top < 0 ? ~top : -1;
            }
        }
        if (overflow) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ANY) lit = !occluded && !overflow;
        else {
            store_hit_record(p, (unsigned)i, hit.geom, hit.id, hit.t, hit.u, hit.v);
            ray_slots[i] = slot;
        }
    }
    if (ANY) film_add_wave(film, pixel, lit, lit ? s.color_r[i] * inv_spp : 0.0f, lit ? s.color_g[i] * inv_spp : 0.0f,
        lit ? s.color_b[i] * inv_spp : 0.0f);
}

template <bool ANY>
__global__ __launch_bounds__(kWave) void k_trace_instanced(SceneDev sc, InstancedDev in, PrimaryStream p, SecondaryStream s,
                                                           const int* size_ptr, int n_value, float* film, float inv_spp,
                                                           unsigned long long* counters, int* err, int* zero_word) {
    __shared__ int stack_lds[kStackCap * kWave];
    trace_instanced_pass<ANY>(sc, in.tlas, StreamStaticEnter{in.instances}, in.ray_slots, p, s, size_ptr, n_value, film, inv_spp,
                              counters, err, zero_word, stack_lds);
}

// ---- the tables an instanced scene derives from its matrices (rodent_hip_scene_create_instanced, rodent_hip_scene_set_transforms) ----
// Every thread owns what it writes; fp32 with every operation rounded on its own (the __f*_rn forms are never contracted).

// One thread per matrix entry: the moved matrices into the descriptor array; the object and id words stay.
__global__ __launch_bounds__(kBlock) void k_instance_matrices(const float* __restrict__ object_to_world, int num_instances,
                                                              RodentInstanceDesc* __restrict__ descs) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 12 * num_instances) return;
    descs[t / 12].object_to_world[t % 12] = object_to_world[t];
}

// One thread per leaf-order slot: slot_of[instance id] = slot.
__global__ __launch_bounds__(kBlock) void k_slot_of(const RodentInstance* __restrict__ instances, int num_instances,
                                                    int* __restrict__ slot_of) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= num_instances) return;
    // (behind a flagged rebuild the instance array is undefined: an id outside the table is written nowhere)
    const int k = instances[j].instance_id & 0x7FFFFFFF;
    if (k < num_instances) slot_of[k] = j;
}

// ((m0 x + m1 y) + m2 z) + m3: the world-box rule of rodent_instances.h
__device__ __forceinline__ float row_point(const float* m, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}
// One thread per world light l, owned by instance k = light_owner[l]: object light l - bases[k].y under k's matrices (rules:
// include/rodent_render.h).  k_motion_world_lights (render_motion.h) states the same statements again -- shared through a function this
// kernel lost a register of its row --: a change here is a change there.
__global__ __launch_bounds__(kBlock) void k_world_lights(const RodentInstanceDesc* __restrict__ descs,
                                                         const RodentInstance* __restrict__ instances, const int* __restrict__ slot_of,
                                                         const int* __restrict__ light_owner, const int2* __restrict__ bases,
                                                         const RodentLight* __restrict__ object_lights, int num_lights,
                                                         RodentLight* __restrict__ lights) {
    const int l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= num_lights) return;
    const int k = light_owner[l];
    const RodentLight src = object_lights[l - bases[k].y];
    const float* m = descs[k].object_to_world;
    const float* w = instances[slot_of[k]].world_to_object;
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

// ---- the tables of the deforming objects D (rodent_hip_scene_deform_device): the steps of render_update.h over D's elements alone ------
// D's triangles are the rows the scene's range table cuts out of the index table (RodentRefitRange: rec_start is the exclusive prefix
// sum of the listed objects' triangle counts, one Tri1 record per triangle); its vertices and lights come as lists the prepare call
// built.  Every thread owns what it writes; whatever lies outside D is not written.
struct DeformTris { const RodentRefitRange* ranges; int num_listed, num_tris; };

// Triangle p of D (p < num_tris) in the index table: the last range whose rec_start is <= p, at most 32 halvings.  The table is the
// scene's own, checked on the host when it was made.
__device__ __forceinline__ int deform_tri(const DeformTris& d, int p) {
    int lo = 0, hi = d.num_listed;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d.ranges[mid].rec_start <= p) lo = mid; else hi = mid;
    }
    return d.ranges[lo].first_tri + (p - d.ranges[lo].rec_start);
}

__global__ __launch_bounds__(kBlock) void k_deform_face_normals(const float4* __restrict__ vertices, const int4* __restrict__ indices,
                                                                DeformTris d, float4* __restrict__ face_normals) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= d.num_tris) return;
    store_face_normal(vertices, indices, deform_tri(d, p), face_normals);
}

// One thread per bound light of D: bound[j] = {object light, the triangle it is bound to}.
__global__ __launch_bounds__(kBlock) void k_deform_light_records(const float4* __restrict__ vertices, const int4* __restrict__ indices,
                                                                 const int2* __restrict__ bound, int num_bound,
                                                                 RodentLight* object_lights) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= num_bound) return;
    store_light_record(vertices, indices, bound[j].y, object_lights[bound[j].x]);
}

// One thread per vertex a triangle of D names: vertex verts[j], its list corner_tri[first[j] .. first[j + 1]) over ALL the scene's
// triangles (a static triangle that shares the vertex contributes its stored face normal).
__global__ __launch_bounds__(kBlock) void k_deform_smooth_normals(const float4* __restrict__ face_normals, const int* __restrict__ verts,
                                                                  const int* __restrict__ first, const int* __restrict__ corner_tri,
                                                                  int num_verts, float4* __restrict__ normals) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= num_verts) return;
    const int end = first[j + 1];
    normals[verts[j]] = smooth_normal(face_normals, corner_tri, first[j], end);
}

__global__ __launch_bounds__(kBlock) void k_deform_tri_shade(const float4* __restrict__ face_normals, const float4* __restrict__ normals,
                                                             const int4* __restrict__ indices, DeformTris d,
                                                             float4* __restrict__ tri_shade) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= d.num_tris) return;
    store_tri_shade(face_normals, normals, indices, deform_tri(d, p), tri_shade);
}
