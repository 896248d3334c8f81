// render_update.h -- the scene's tables after its vertices moved, derived on the device (included by render.hip after render_sort.h).
#pragma once
// ---- rodent_hip_scene_refit_device: what the scene keeps from positions (rules: include/rodent_render.h, "moved geometry") ----------
// Five kernels around the in-place refit (rodent_hip_refit_bvh2_tri1): k_face_normals and k_light_records read the moved vertices,
// k_smooth_normals sums the face normals of a vertex's corners in the fixed order of its incidence list, k_tri_shade gathers the shading
// records, k_scene_images rebuilds both LDS top images from the refitted nodes.  Every thread owns what it writes: no thread waits for
// another, no arrival counters, no floating-point atomics; every value is a function of the inputs alone.  All arithmetic is fp32 with
// every operation rounded on its own (the __f*_rn forms are never contracted), as host/vec.h computes it.  The square root is sqrtf,
// correctly rounded like the shader's len(): __fsqrt_rn is the hardware's approximate instruction with this toolchain's headers.

struct UpdateV3 { float x, y, z; };

// (v1 - v0) x (v2 - v0) of triangle `t`, host/vec.h's cross; the corners through `v`.
__device__ __forceinline__ UpdateV3 corner_cross(const float4* __restrict__ vertices, const int4 ix, float4 v[3]) {
    v[0] = vertices[ix.x]; v[1] = vertices[ix.y]; v[2] = vertices[ix.z];
    const float ax = __fsub_rn(v[1].x, v[0].x), ay = __fsub_rn(v[1].y, v[0].y), az = __fsub_rn(v[1].z, v[0].z);
    const float bx = __fsub_rn(v[2].x, v[0].x), by = __fsub_rn(v[2].y, v[0].y), bz = __fsub_rn(v[2].z, v[0].z);
    return {__fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by)), __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz)),
            __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx))};
}
// host/vec.h's dot(a, a): (x x + y y) + z z
__device__ __forceinline__ float length2(float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
}

// Triangle t's face normal: c * (1 / |c|), w = 0.  A degenerate triangle gives NaN, as on the host.
__device__ __forceinline__ void store_face_normal(const float4* __restrict__ vertices, const int4* __restrict__ indices, int t,
                                                  float4* __restrict__ face_normals) {
    float4 v[3];
    const UpdateV3 c = corner_cross(vertices, indices[t], v);
    const float inv = __fdiv_rn(1.0f, sqrtf(length2(c.x, c.y, c.z)));
    face_normals[t] = make_float4(__fmul_rn(c.x, inv), __fmul_rn(c.y, inv), __fmul_rn(c.z, inv), 0.0f);
}

// One thread per triangle.
__global__ __launch_bounds__(kBlock) void k_face_normals(const float4* __restrict__ vertices, const int4* __restrict__ indices,
                                                         int num_tris, float4* __restrict__ face_normals) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= num_tris) return;
    store_face_normal(vertices, indices, t, face_normals);
}

// Light L from the triangle t it is bound to: corners, normal and 1 / area.  The fourth word of every corner and the colour stay as
// stored.
__device__ __forceinline__ void store_light_record(const float4* __restrict__ vertices, const int4* __restrict__ indices, int t,
                                                   RodentLight& L) {
    float4 v[3];
    const UpdateV3 c = corner_cross(vertices, indices[t], v);
    const float l = sqrtf(length2(c.x, c.y, c.z)), inv = __fdiv_rn(1.0f, l);
    L.v0[0] = v[0].x; L.v0[1] = v[0].y; L.v0[2] = v[0].z;
    L.v1[0] = v[1].x; L.v1[1] = v[1].y; L.v1[2] = v[1].z;
    L.v2[0] = v[2].x; L.v2[1] = v[2].y; L.v2[2] = v[2].z;
    *reinterpret_cast<float4*>(L.n) = make_float4(__fmul_rn(c.x, inv), __fmul_rn(c.y, inv), __fmul_rn(c.z, inv),
                                                  __fdiv_rn(1.0f, __fmul_rn(0.5f, l)));
}

// One thread per light: the record of the triangle it is bound to (light_tri[k], -1: the light keeps its bytes).
__global__ __launch_bounds__(kBlock) void k_light_records(const float4* __restrict__ vertices, const int4* __restrict__ indices,
                                                          const int* __restrict__ light_tri, int num_lights, RodentLight* lights) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= num_lights) return;
    const int t = light_tri[k];
    if (t < 0) return;
    store_light_record(vertices, indices, t, lights[k]);
}

// A vertex's normal from its incidence list corner_tri[begin .. end): the face normals of its corners summed in list order (ascending
// (triangle, corner)), then the loader's normalisation.  A triangle that names the vertex twice is in the list twice.
__device__ __forceinline__ float4 smooth_normal(const float4* __restrict__ face_normals, const int* __restrict__ corner_tri, int begin,
                                                int end) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int j = begin; j < end; j++) {
        const float4 n = face_normals[corner_tri[j]];
        sx = __fadd_rn(sx, n.x); sy = __fadd_rn(sy, n.y); sz = __fadd_rn(sz, n.z);
    }
    const float l2 = length2(sx, sy, sz);
    float4 out = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
    if (l2 > 1.1920928955078125e-7f) {                    // FLT_EPSILON; a NaN fails the comparison and takes (0, 1, 0) too
        const float inv = __fdiv_rn(1.0f, sqrtf(l2));
        out = make_float4(__fmul_rn(sx, inv), __fmul_rn(sy, inv), __fmul_rn(sz, inv), 0.0f);
    }
    return out;
}

// One thread per vertex; the list of vertex v is corner_tri[first[v] .. first[v + 1]).
__global__ __launch_bounds__(kBlock) void k_smooth_normals(const float4* __restrict__ face_normals, const int* __restrict__ first,
                                                           const int* __restrict__ corner_tri, int num_vertices,
                                                           float4* __restrict__ normals) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= num_vertices) return;
    const int end = first[v + 1];
    normals[v] = smooth_normal(face_normals, corner_tri, first[v], end);
}

// The SceneDev::tri_shade record of triangle t (face normal, then the three corners' vertex normals) as three 16-byte stores.
__device__ __forceinline__ void store_tri_shade(const float4* __restrict__ face_normals, const float4* __restrict__ normals,
                                                const int4* __restrict__ indices, int t, float4* __restrict__ tri_shade) {
    const int4 ix = indices[t];
    const float4 f = face_normals[t], a = normals[ix.x], b = normals[ix.y], c = normals[ix.z];
    float4* o = tri_shade + 3 * (size_t)t;
    o[0] = make_float4(f.x, f.y, f.z, a.x);
    o[1] = make_float4(a.y, a.z, b.x, b.y);
    o[2] = make_float4(b.z, c.x, c.y, c.z);
}

// One thread per triangle.
__global__ __launch_bounds__(kBlock) void k_tri_shade(const float4* __restrict__ face_normals, const float4* __restrict__ normals,
                                                      const int4* __restrict__ indices, int num_tris, float4* __restrict__ tri_shade) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= num_tris) return;
    store_tri_shade(face_normals, normals, indices, t, tri_shade);
}

// One wave per image (block 0: kSceneTopNodes records, block 1: kPersistTopNodes), the slots' node ids in LDS: the bytes of the host's
// build_image() (render.hip), level by level.  A round holds the slots [begin, end) of one level in queue order; the slot of child j of
// its i-th node is the count of slots taken so far plus the inner children of the round's earlier nodes (plus in0 for j = 1), and a child
// gets it only while it is below the capacity -- the order in which the host's queue hands slots out.  (build_top_image of
// traversal_device.h numbers a round's first children before its second children: another image.)
__global__ __launch_bounds__(kWave) void k_scene_images(const Node2* __restrict__ nodes, int4* __restrict__ image_small,
                                                        int4* __restrict__ image_large) {
    __shared__ int slot_node[kPersistTopNodes];
    const int capacity = blockIdx.x ? kPersistTopNodes : kSceneTopNodes;
    int4* const image = blockIdx.x ? image_large : image_small;
    const int lane = threadIdx.x;
    if (lane == 0) slot_node[0] = 1;
    __syncthreads();
    int begin = 0, end = 1;
    while (begin < end) {
        int taken = end;                                   // slots handed out so far (not capped: a slot >= capacity is refused)
        for (int base = begin; base < end; base += kWave) {
            const int slot = base + lane;
            const bool on = slot < end;
            int4 r0 = {}, r1 = {}, r2 = {}, r3 = {};
            int id = 0;
            if (on) {
                id = slot_node[slot];
                const int4* p = reinterpret_cast<const int4*>(nodes + (id - 1));
                r0 = p[0]; r1 = p[1]; r2 = p[2]; r3 = p[3];
            }
            const bool in0 = on && r3.x > 0, in1 = on && r3.y > 0;       // r3.x / r3.y = Node2::child
            const unsigned long long m0 = __ballot(in0), m1 = __ballot(in1), below = (1ull << lane) - 1ull;
            const int s0 = taken + __popcll(m0 & below) + __popcll(m1 & below), s1 = s0 + (in0 ? 1 : 0);
            if (in0 && s0 < capacity) { slot_node[s0] = r3.x; r3.x = kLdsTag + s0 * (int)sizeof(Node2); }
            if (in1 && s1 < capacity) { slot_node[s1] = r3.y; r3.y = kLdsTag + s1 * (int)sizeof(Node2); }
            taken += __popcll(m0) + __popcll(m1);
            if (on) { r3.z = id; r3.w = 0; int4* q = image + 4 * slot; q[0] = r0; q[1] = r1; q[2] = r2; q[3] = r3; }
        }
        __syncthreads();
        begin = end; end = min(capacity, taken);
    }
    const int4 zero = {0, 0, 0, 0};
    for (int j = 4 * end + lane; j < 4 * capacity; j += kWave) image[j] = zero;       // unused records: all zero
}
