// render_trace.h -- the renderer's stream traversal stage (K1 / K6): the LDS stacks, the single-step loops trace_one / trace_two, the
// stream ray and hit-record accessors, and the five kernel families k_trace_primary / _secondary / _persist / _refill / _deep.
//
// Included by render.hip inside its anonymous namespace (after the constants, stream_size and k_generate).
#pragma once

// ---------------------------------------------------------------------------------------------
// K1 / K6: BVH2 traversal over an SoA ray stream.  Per-ray visit order = the reference kernel
// (traversal/mapping_gpu.impala:94-178); wave scheduling = the single-step loop of traversal.hip
// (branch-free node step).  Stack: 16-entry window in LDS; deeper rays go to k_trace_deep (stream kernels) / scratch (megakernel).
// ---------------------------------------------------------------------------------------------
constexpr int kLdsStack = 16;
constexpr int kPersistWaves = 16;               // waves per workgroup of the persistent traversal kernels (k_trace_persist, k_trace_refill)
constexpr int kSpillEntries = kStackCap - kLdsStack;
// Stack of the megakernel (one workgroup per film tile): 16-entry window in LDS, deeper entries in scratch.
struct StreamStack {
    lds_int* col; int* err;
    int local[kSpillEntries];
    __device__ __forceinline__ int get(int e) const {
        if (__builtin_expect(e < kLdsStack, 1)) return col[e * kWave];
        return local[(e < kStackCap ? e : kStackCap - 1) - kLdsStack];
    }
    __device__ __forceinline__ void put(int e, int v) {
        if (__builtin_expect(e < kLdsStack, 1)) col[e * kWave] = v;
        else if (e < kStackCap) local[e - kLdsStack] = v;
        else *err = 1;
    }
};

// LDS-only stack of the stream traversal kernels, kept as a cursor (pointer to the entry under the top).  A ray whose
// stack outgrows the 16-entry window is abandoned (overflow = true) and traced again by k_trace_deep with the
// 64-entry stack in global memory -- the arrangement of traversal.hip (k_bvh2_single / k_bvh2_finish): no overflow
// handling inside the hot loop.
// The persistent kernels (k_trace_persist, k_trace_refill) do not abandon it: the oldest entries move to the wave's block of global memory
// and the ray goes on in its lane (SPILLW = the window's rows; stack_spill / stack_reload, traversal_device.h).
struct CursorStack {
    lds_int* sp; lds_int* limit; bool overflow;
    int* spill; int* err;                          // the launch's spill buffer (wave-uniform) and error flag
    __device__ __forceinline__ void init(lds_int* col, int window = kLdsStack, int* spill_ = nullptr, int* err_ = nullptr) {
        sp = col; limit = col + window * kWave; overflow = false; col[0] = 0; spill = spill_; err = err_;
    }
};
// 64 entries ([entry][lane]), the reference's capacity (stack.impala:53), in 16 KB of LDS; used by k_trace_deep only.  (In global
// memory, rounds 1-2, every push and pop was a round trip: ~100 us for the first deep ray of a launch.)
struct DeepStack {
    lds_int* base; int* err;
    __device__ __forceinline__ int get(int e) const { return base[(e < kStackCap ? e : kStackCap - 1) * kWave]; }
    __device__ __forceinline__ void put(int e, int v) { if (e < kStackCap) base[e * kWave] = v; else *err = 1; }
};
template <typename T> struct is_cursor { static constexpr bool value = false; };
template <> struct is_cursor<CursorStack> { static constexpr bool value = true; };

// XCD-aware wave -> chunk mapping of traversal.hip (k_bvh2_single): groups of 32 consecutive 64-ray chunks per XCD.
__device__ __forceinline__ int xcd_chunk(int block, int total_chunks) {
    constexpr int G = 32;
    const int span = 8 * G, full = (total_chunks / span) * span;
    if (block >= full) return block;
    const int x = block % 8, l = block / 8;
    return ((l / G) * 8 + x) * G + l % G;
}

struct StreamHit { int prim, geom; float t, u, v; };

// Film accumulation for a wavefront (mapping_gpu.impala:32-45 does one atomic per ray and channel).
// With spp > 1 the rays of one pixel sit in neighbouring lanes, and 64 lanes hitting the same three
// addresses serialise in the atomic unit (measured: the shadow pass took 4x the primary pass on the
// Cornell box).  Lanes that share a pixel are therefore summed in the wave first (butterfly over the
// lanes, a fixed order) and one lane issues the atomics; after kFilmRounds distinct pixels the remaining
// lanes fall back to their own atomics.  Only the order of the fp32 additions differs from the reference.
constexpr int kFilmRounds = 4;
__device__ __forceinline__ void film_add_wave(float* film, int pixel, bool valid, float r, float g, float b) {
    unsigned long long todo = __ballot(valid);
    for (int round = 0; round < kFilmRounds && todo; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const int p0 = __shfl(pixel, leader);
        const bool mine = valid && pixel == p0;
        const unsigned long long same = __ballot(mine);
        if (__popcll(same) > 1) {
            float sr = mine ? r : 0.0f, sg = mine ? g : 0.0f, sb = mine ? b : 0.0f;
            for (int o = 32; o > 0; o >>= 1) { sr += __shfl_xor(sr, o); sg += __shfl_xor(sg, o); sb += __shfl_xor(sb, o); }
            if ((int)(threadIdx.x % kWave) == leader) { float* px = film + 3 * (size_t)p0; unsafeAtomicAdd(px, sr);
                unsafeAtomicAdd(px + 1, sg); unsafeAtomicAdd(px + 2, sb); }
            if (mine) valid = false;
        } else if (mine) {
            float* px = film + 3 * (size_t)pixel; unsafeAtomicAdd(px, r); unsafeAtomicAdd(px + 1, g); unsafeAtomicAdd(px + 2, b);
            valid = false;
        }
        todo &= ~same;
    }
    if (valid) { float* px = film + 3 * (size_t)pixel; unsafeAtomicAdd(px, r); unsafeAtomicAdd(px + 1, g); unsafeAtomicAdd(px + 2, b); }
}

// Single-step schedule, as k_bvh2_single / unified_chunk in traversal.hip: each lane advances by one node step or
// one triangle test per wave iteration and the loads of both kinds are in flight together.
// on_hit(prim, geom, t, u, v) is called for every accepted triangle (the last call is the closest hit); returns whether
// anything was hit.  The stream kernels store from on_hit instead of carrying a hit record in registers.
// TOP: `image` is the scene's top-of-tree image staged in LDS by the workgroup (traversal_device.h); a node id >= kLdsTag is a
// link into it and is fetched with ds_read_b128 instead of through the vector-memory pipeline.
template <bool ANY, bool TOP = false, int SPILLW = 0, typename Stack, typename OnHit>
__device__ __forceinline__ bool trace_one(const Node2* __restrict__ nodes, const Tri1* __restrict__ tris, RayX ray, Stack& st,
    OnHit on_hit, lds_int* image = nullptr) {
    constexpr bool kCursor = is_cursor<Stack>::value;
    bool any_found = false;
    int ptr = 0, top = TOP ? kLdsTag : 1;
    if constexpr (!kCursor) st.put(0, 0);
    ray.tmin = canonical(ray.tmin); ray.tmax = canonical(ray.tmax);           // see slab_canonical (traversal_device.h)
    // both bases as integers in VGPRs for the per-lane select, then GLOBAL pointers again (see unified_chunk)
    typedef const __attribute__((address_space(1))) char* gptr;
    // node ids are 1-based
    unsigned long long node_bits = reinterpret_cast<unsigned long long>(nodes - 1), tri_bits = reinterpret_cast<unsigned long long>(tris);
    asm volatile("" : "+v"(node_bits), "+v"(tri_bits));
    const gptr node_base = (gptr)node_bits, tri_base = (gptr)tri_bits;
    while (__ballot(top != 0)) {
        if (top != 0) {
            const bool is_node = top > 0;
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            typedef int i32x2 __attribute__((ext_vector_type(2)));
            f32x4 q0, q1, q2;
            i32x2 ch;
            int popped;
            if constexpr (TOP && kCursor) {
                // both kinds of fetch -- LDS image, memory -- and the word under the cursor in flight together (joint_fetch,
                // traversal_device.h)
                const unsigned idx = (unsigned)(is_node ? top : ~top), stride = is_node ? (unsigned)sizeof(Node2) : (unsigned)sizeof(Tri1);
                const gptr addr = (is_node ? node_base : tri_base) + (size_t)idx * stride;
                joint_fetch(q0, q1, q2, ch, popped, top >= kLdsTag, (unsigned)(size_t)image + (unsigned)(top - kLdsTag), addr,
                    addr + (is_node ? 48u : 40u), st.sp);
            } else {
                const unsigned idx = (unsigned)(is_node ? top : ~top), stride = is_node ? (unsigned)sizeof(Node2) : (unsigned)sizeof(Tri1);
                const gptr addr = (is_node ? node_base : tri_base) + (size_t)idx * stride;
                const __attribute__((address_space(1))) f32x4* p = (const __attribute__((address_space(1))) f32x4*)addr;
                q0 = p[0]; q1 = p[1]; q2 = p[2];
                // child ids / (triangle lanes) own last 8 bytes
                ch = *(const __attribute__((address_space(1))) i32x2*)(addr + (is_node ? 48u : 40u));
                if constexpr (kCursor) popped = *st.sp; else popped = st.get(ptr);
                // keep all four loads in flight together (see unified_chunk)
                asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(ch));
            }
            if (is_node) {
                float te0, te1;
                const bool h0 = slab_canonical(ray, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, te0) && ch.x != 0;
                const bool h1 = slab_canonical(ray, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, te1) && ch.y != 0;
                // (any-hit rays -- the renderer's shadow rays -- take child 0 first: occlusion does not depend on the order, see
                // k_trace_refill's SHADOW_ORDER)
                const bool c0first = ANY ? true : te0 < te1, both = h0 && h1;
                top = both ? (c0first ? ch.x : ch.y) : (h0 ? ch.x : (h1 ? ch.y : popped));
                if constexpr (kCursor) {
                    st.sp[kWave] = c0first ? ch.y : ch.x;
                    st.sp += (both ? kWave : 0) - ((h0 || h1) ? 0 : kWave);
                    // (`both`: popping the sentinel moves sp below its column)
                    if (both && st.sp >= st.limit) {
                        if constexpr (SPILLW > 0) stack_spill<SPILLW>(st.sp, top, st.limit, st.spill, kPersistWaves, st.err);
                        else { st.overflow = true; top = 0; }
                    }
                } else {
                    st.put(ptr + 1, c0first ? ch.y : ch.x);
                    ptr += (both ? 1 : 0) - ((h0 || h1) ? 0 : 1);
                }
            } else {
                const int prim_id = __float_as_int(q2.w);
                const float nx = cross_x(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z), ny = cross_y(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z),
                    nz = cross_z(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z);
                float t, u, v;
                bool found = false;
                if (intersect_tri(ray, q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z, nx, ny, nz, t, u, v)) {
                    on_hit(prim_id & 0x7FFFFFFF, __float_as_int(q1.w), t, u, v);
                    ray.tmax = t; found = true; any_found = true;
                }
                const bool leave = prim_id < 0;                               // sentinel: the leaf is done
                top = (ANY && found) ? 0 : (leave ? popped : top - 1);        // top - 1 == ~(j + 1)
                if constexpr (kCursor) st.sp -= (leave && !(ANY && found)) ? kWave : 0;
                else ptr -= (leave && !(ANY && found)) ? 1 : 0;
            }
            // popped row 0 while entries are out
            if constexpr (kCursor && SPILLW > 0) if (top >= kSpillMark) stack_reload<SPILLW>(st.sp, top, st.limit, st.spill, kPersistWaves);
        }
    }
    return any_found;
}

// intersection.impala:88-99
__device__ __forceinline__ RayX make_rayx(float ox, float oy, float oz, float dx, float dy, float dz, float tmin, float tmax) {
    RayX x;
    x.ox = ox; x.oy = oy; x.oz = oz; x.dx = dx; x.dy = dy; x.dz = dz; x.tmin = tmin; x.tmax = tmax;
    x.idx = safe_rcp(x.dx); x.idy = safe_rcp(x.dy); x.idz = safe_rcp(x.dz);
    x.iox = -(x.ox * x.idx); x.ioy = -(x.oy * x.idy); x.ioz = -(x.oz * x.idz);
    return x;
}
// Two rays per lane, back to back, in ONE wave-level loop (the megakernel's joint form): first the shadow ray `a` (any hit:
// the first accepted triangle ends it), then the path ray `b` (closest hit, on_hit_b for every accepted triangle), both from
// the same origin.  A wave then needs max over its lanes of (steps of a + steps of b) iterations instead of the sum of the two
// maxima of separate loops.  Per ray the visit order is trace_one's.  Returns {a was occluded, b hit something}.
struct TwoHits { bool a_occluded, b_hit; };
template <typename Stack, typename OnHit>
__device__ __forceinline__ TwoHits trace_two(const Node2* __restrict__ nodes, const Tri1* __restrict__ tris, bool has_a, bool has_b,
                                             float ox, float oy, float oz, float adx, float ady, float adz, float a_tmin, float a_tmax,
                                             float bdx, float bdy, float bdz, float b_tmin, float b_tmax, Stack& st, OnHit on_hit_b) {
    TwoHits out{false, false};
    bool phase_a = has_a;
    RayX ray = phase_a ? make_rayx(ox, oy, oz, adx, ady, adz, a_tmin, a_tmax) : make_rayx(ox, oy, oz, bdx, bdy, bdz, b_tmin, b_tmax);
    ray.tmin = canonical(ray.tmin); ray.tmax = canonical(ray.tmax);
    int ptr = 0, top = (has_a || has_b) ? 1 : 0;
    st.put(0, 0);
    typedef const __attribute__((address_space(1))) char* gptr;
    unsigned long long node_bits = reinterpret_cast<unsigned long long>(nodes - 1), tri_bits = reinterpret_cast<unsigned long long>(tris);
    asm volatile("" : "+v"(node_bits), "+v"(tri_bits));
    const gptr node_base = (gptr)node_bits, tri_base = (gptr)tri_bits;
    for (;;) {
        // a lane whose shadow ray is finished goes on with its path ray (if it has one)
        const bool next = top == 0 && phase_a;
        if (__ballot(next)) {
            if (next) {
                phase_a = false;
                if (has_b) {
                    ray = make_rayx(ox, oy, oz, bdx, bdy, bdz, b_tmin, b_tmax);
                    ray.tmin = canonical(ray.tmin); ray.tmax = canonical(ray.tmax);
                    top = 1; ptr = 0; st.put(0, 0);
                }
            }
        }
        if (!__ballot(top != 0)) break;
        if (top != 0) {
            const bool is_node = top > 0;
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            typedef int i32x2 __attribute__((ext_vector_type(2)));
            const unsigned idx = (unsigned)(is_node ? top : ~top), stride = is_node ? (unsigned)sizeof(Node2) : (unsigned)sizeof(Tri1);
            const gptr addr = (is_node ? node_base : tri_base) + (size_t)idx * stride;
            const __attribute__((address_space(1))) f32x4* p = (const __attribute__((address_space(1))) f32x4*)addr;
            f32x4 q0 = p[0], q1 = p[1], q2 = p[2];
            i32x2 ch = *(const __attribute__((address_space(1))) i32x2*)(addr + (is_node ? 48u : 40u));
            const int popped = st.get(ptr);
            asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(ch));
            if (is_node) {
                float te0, te1;
                const bool h0 = slab_canonical(ray, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, te0) && ch.x != 0;
                const bool h1 = slab_canonical(ray, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, te1) && ch.y != 0;
                const bool c0first = te0 < te1, both = h0 && h1;
                top = both ? (c0first ? ch.x : ch.y) : (h0 ? ch.x : (h1 ? ch.y : popped));
                st.put(ptr + 1, c0first ? ch.y : ch.x);
                ptr += (both ? 1 : 0) - ((h0 || h1) ? 0 : 1);
            } else {
                const int prim_id = __float_as_int(q2.w);
                const float nx = cross_x(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z), ny = cross_y(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z),
                    nz = cross_z(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z);
                float t, u, v;
                bool ends = false;
                if (intersect_tri(ray, q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z, nx, ny, nz, t, u, v)) {
                    if (phase_a) { out.a_occluded = true; ends = true; }
                    else { on_hit_b(prim_id & 0x7FFFFFFF, __float_as_int(q1.w), t, u, v); ray.tmax = t; out.b_hit = true; }
                }
                const bool leave = prim_id < 0;
                top = ends ? 0 : (leave ? popped : top - 1);
                ptr -= (leave && !ends) ? 1 : 0;
            }
        }
    }
    return out;
}

__device__ __forceinline__ RayX load_stream_ray(const RayStream& r, int i) {   // driver.impala:63-84
    return make_rayx(r.org_x[i], r.org_y[i], r.org_z[i], r.dir_x[i], r.dir_y[i], r.dir_z[i], r.tmin[i], r.tmax[i]);
}

// Hit records of a primary stream.  The ABI's layout (driver.impala:24-61) is five arrays -- geom_id, prim_id, t, u, v -- and a record is
// five 4-byte stores into five different 32-byte sectors; lanes that were refilled hold non-consecutive rays, so nothing coalesces: the
// traversal launches of the atrium frame wrote 97 bytes per ray for <= 20 bytes of records (profiles/r03_render_profile_cfg5.json).  Inside
// the library's own loop (render_rows; PrimaryStream::pad bit 0, never set on a caller's stream) the SAME memory -- the five arrays are
// consecutive in the slab, carve_primary -- holds one 20-byte record per ray at words [5 i, 5 i + 5): one 16-byte and one 4-byte store into
// one or two sectors; the shader reads the records in stream order (coalesced).  Record fields: geom_id = num_geometries on a miss
// (driver.impala:106-115).
constexpr int kHitRecordsAoS = 1;
struct HitRecord { int geom, prim; float t, u, v; };
typedef int i32x4_dword_aligned __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store_hit_record(const PrimaryStream& p, unsigned i, int geom, int prim, float t, float u, float v) {
    if (p.pad & kHitRecordsAoS) {
        int* rec = p.geom_id + 5u * i;
        *reinterpret_cast<i32x4_dword_aligned*>(rec) = i32x4_dword_aligned{geom, prim, __float_as_int(t), __float_as_int(u)};
        rec[4] = __float_as_int(v);
    } else { p.geom_id[i] = geom; p.prim_id[i] = prim; p.t[i] = t; p.u[i] = u; p.v[i] = v; }
}
__device__ __forceinline__ HitRecord load_hit_record(const PrimaryStream& p, unsigned i) {
    if (p.pad & kHitRecordsAoS) {
        const int* rec = p.geom_id + 5u * i;
        const i32x4_dword_aligned q = *reinterpret_cast<const i32x4_dword_aligned*>(rec);
        return HitRecord{q.x, q.y, __int_as_float(q.z), __int_as_float(q.w), __int_as_float(rec[4])};
    }
    return HitRecord{p.geom_id[i], p.prim_id[i], p.t[i], p.u[i], p.v[i]};
}
__device__ __forceinline__ int load_hit_geom(const PrimaryStream& p, unsigned i) {
    return (p.pad & kHitRecordsAoS) ? p.geom_id[5u * i] : p.geom_id[i]; }

// primary: writes the hit record (geom_id = num_geometries on a miss, driver.impala:106-115; prim_id, t, u, v)
template <bool TOP = false, int SPILLW = 0>
__device__ __forceinline__ void trace_primary_ray(const SceneDev& sc, const PrimaryStream& p, int i, CursorStack* cursor, DeepStack* deep,
    lds_int* image = nullptr) {
    const RayX ray = load_stream_ray(p.rays, i);
    store_hit_record(p, (unsigned)i, sc.num_materials, -1, ray.tmax, 0.0f, 0.0f);     // the miss record; hits overwrite it
    auto on_hit = [&](int prim, int geom, float t, float u, float v) {
        unsigned k = (unsigned)i;
        // opaque index: SGPR bases + one VGPR offset here, instead of five 64-bit addresses held across the loop
        asm volatile("" : "+v"(k));
        store_hit_record(p, k, geom, prim, t, u, v);
    };
    if (cursor) trace_one<false, TOP, SPILLW>(sc.nodes, sc.tris, ray, *cursor, on_hit, image);
    else trace_one<false>(sc.nodes, sc.tris, ray, *deep, on_hit);
}

// WAVES x 64 threads per workgroup; TOPN > 0: the scene's top-of-tree image (first TOPN records) is staged in LDS behind the
// WAVES stack windows (kTopStack entries each then: 2 x 4 KB + 31 x 64 B = 16 workgroups per CU, all 32 wave slots).
constexpr int kTopStack = 15, kSceneTopNodes = 31, kTraceWaves = 2;
// below one resident generation of rays the persistent form does not pay (traversal.hip)
constexpr int kPersistMinRays = 8192 * kWave;
template <int WAVES, int TOPN>
__device__ __forceinline__ lds_int* stage_scene_image(const SceneDev& sc, int* lds, int& chunk, int total_chunks) {
    constexpr int kWindow = TOPN ? kTopStack : kLdsStack;
    lds_int* image = (lds_int*)lds + WAVES * (kWindow + 1) * kWave;
    if (TOPN) {
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        for (int j = threadIdx.x; j < TOPN * 4; j += WAVES * kWave)
            reinterpret_cast<__attribute__((address_space(3))) i32x4*>(image)[j] = reinterpret_cast<const i32x4*>(sc.top_image)[j];
    }
    // XCD-aware wave -> chunk mapping (xcd_chunk): wave l of XCD x, l counted over the workgroups of that XCD
    const int wave = threadIdx.x / kWave;
    constexpr int G = 32;
    const int span = 8 * G, full = (total_chunks / span) * span;
    chunk = blockIdx.x * WAVES + wave;
    if ((int)blockIdx.x * WAVES < full) {
        const int x = blockIdx.x % 8, l = (blockIdx.x / 8) * WAVES + wave;
        chunk = ((l / G) * 8 + x) * G + l % G;
    }
    if (TOPN && WAVES > 1) __syncthreads();
    return image;
}

template <int WAVES, int TOPN>
__global__ __launch_bounds__(kWave * WAVES) void k_trace_primary(SceneDev sc, PrimaryStream p, const int* size_ptr, int n_value,
    int* deep_count, unsigned long long* counters,
                                                                 int* deep_list) {
    constexpr int kWindow = TOPN ? kTopStack : kLdsStack;
    __shared__ __attribute__((aligned(16))) int lds[WAVES * (kWindow + 1) * kWave + TOPN * 16];
    const int n = stream_size(size_ptr, n_value);
    int chunk;
    lds_int* image = stage_scene_image<WAVES, TOPN>(sc, lds, chunk, (n + kWave - 1) / kWave);
    const int lane = threadIdx.x % kWave, i = chunk * kWave + lane;
    if (i >= n) return;
    CursorStack st; st.init((lds_int*)lds + (threadIdx.x / kWave) * (kWindow + 1) * kWave + lane, kWindow);
    trace_primary_ray<(TOPN > 0)>(sc, p, i, &st, nullptr, image);
    if (st.overflow) deep_list[atomicAdd(deep_count, 1)] = i;
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(&counters[0], (unsigned long long)n);
}

// secondary: any-hit; unoccluded rays add their colour to the film (mapping_gpu.impala:32-45,47-80)
template <int WAVES, int TOPN>
__global__ __launch_bounds__(kWave * WAVES) void k_trace_secondary(SceneDev sc, SecondaryStream s, const int* size_ptr, int n_value,
    float* film, float inv_spp,
                                                                   int* deep_count, unsigned long long* counters, int* deep_list) {
    constexpr int kWindow = TOPN ? kTopStack : kLdsStack;
    __shared__ __attribute__((aligned(16))) int lds[WAVES * (kWindow + 1) * kWave + TOPN * 16];
    const int n = stream_size(size_ptr, n_value);
    int chunk;
    // (the grid covers n_value rays: the mapping must not depend on the device-side n)
    lds_int* image = stage_scene_image<WAVES, TOPN>(sc, lds, chunk, (n_value + kWave - 1) / kWave);
    const int lane = threadIdx.x % kWave, i = chunk * kWave + lane;
    if (chunk * kWave >= n) return;
    const int pixel = i < n ? s.rays.id[i] : -1;
    const unsigned long long live = __ballot(pixel >= 0);
    // striped over 64 words: one counter word saturates near 88 atomics/us and made this kernel 3x slower
    if (lane == 0 && live) atomicAdd(&counters[4 + (chunk & 63)], (unsigned long long)__popcll(live));
    bool lit = false;
    if (pixel >= 0) {
        CursorStack st; st.init((lds_int*)lds + (threadIdx.x / kWave) * (kWindow + 1) * kWave + lane, kWindow);
        lit = !trace_one<true, (TOPN > 0)>(sc.nodes, sc.tris, load_stream_ray(s.rays, i), st, [](int, int, float, float, float) {}, image);
        if (st.overflow) { deep_list[atomicAdd(deep_count, 1)] = i; lit = false; }      // k_trace_deep decides
    }
    film_add_wave(film, pixel, lit, lit ? s.color_r[i] * inv_spp : 0.0f, lit ? s.color_g[i] * inv_spp : 0.0f,
        lit ? s.color_b[i] * inv_spp : 0.0f);
}

// Persistent form of the two kernels above (rodent_hip_render_trace_persistent; traversal.hip k_bvh2_top_persist): one resident
// generation of 16-wave workgroups, each stages the scene's 255-record image once and its waves draw 64-ray chunks from 64
// striped ticket counters (ticket t of stripe s = chunk ((t / 32) * 64 + s) * 32 + t % 32; a wave's first ticket is its rank in
// the stripe).  The stream size may live on the device: the grid does not depend on it.  k_trace_deep zeroes the counters.
constexpr int kPersistTopNodes = 255, kTraceStripes = 64, kTraceCounterStride = 16;
// MODE 0: the closest-hit pass over `p`; 1: the shadow pass over `s`; 2 ("joint", rodent_hip_render_trace_persistent(dev, 2)): BOTH in
// one launch -- the closest-hit pass of an iteration and the shadow pass of the iteration before it depend on the same shader
// run and on nothing else, so their chunks go through one ticket sequence (the closest-hit chunks first): one resident
// generation works through both lists, no pass waits for the other's tail, and there is no second stream whose kernels a
// persistent grid would shut out.
template <int MODE>
__global__ __launch_bounds__(kWave * kPersistWaves) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_trace_persist(SceneDev sc, PrimaryStream p, int n_primary, SecondaryStream s, const int* size_ptr, int n_value, float* film,
    float inv_spp,
                     int* deep_count_primary, int* deep_count_secondary, unsigned long long* counters, int* deep_list_primary,
                         int* deep_list_secondary, int* tickets,
                     int* spill, int* err) {
    constexpr int kStackInts = kPersistWaves * (kTopStack + 1) * kWave;
    __shared__ __attribute__((aligned(16))) int lds[kStackInts + kPersistTopNodes * 16];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    lds_int* image = (lds_int*)lds + kStackInts;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    for (int j = threadIdx.x; j < kPersistTopNodes * 4; j += kWave * kPersistWaves)
        reinterpret_cast<__attribute__((address_space(3))) i32x4*>(image)[j] = reinterpret_cast<const i32x4*>(sc.top_image_large)[j];
    const int np = MODE == 1 ? 0 : n_primary, ns = MODE == 0 ? 0 : stream_size(size_ptr, n_value);
    const int chunks_p = (np + kWave - 1) / kWave, total_chunks = chunks_p + (ns + kWave - 1) / kWave;
    const int stripe = blockIdx.x % kTraceStripes, stripe_waves = (gridDim.x / kTraceStripes) * kPersistWaves;
    int* counter = tickets + stripe * kTraceCounterStride;
    // the wave's rank in its stripe, wave-major (traversal_top.h stripe_rank)
    int t = wave * ((int)gridDim.x / kTraceStripes) + (int)blockIdx.x / kTraceStripes;
    lds_int* col = (lds_int*)lds + wave * (kTopStack + 1) * kWave + lane;
    __syncthreads();
    if (MODE != 1 && threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(&counters[0], (unsigned long long)np);
    for (;;) {
        const int group_first = ((t / 32) * kTraceStripes + stripe) * 32, chunk = group_first + t % 32;
        if (group_first >= total_chunks) break;
        if (chunk < chunks_p) {
            const int i = chunk * kWave + lane;
            if (i < np) {
                CursorStack st; st.init(col, kTopStack, spill, err);
                trace_primary_ray<true, kTopStack>(sc, p, i, &st, nullptr, image);
            }
        } else if (chunk < total_chunks) {
            const int c = chunk - chunks_p, i = c * kWave + lane;
            const int pixel = i < ns ? s.rays.id[i] : -1;
            const unsigned long long live = __ballot(pixel >= 0);
            if (lane == 0 && live) atomicAdd(&counters[4 + (c & 63)], (unsigned long long)__popcll(live));
            bool lit = false;
            if (pixel >= 0) {
                CursorStack st; st.init(col, kTopStack, spill, err);
                lit = !trace_one<true, true, kTopStack>(sc.nodes, sc.tris, load_stream_ray(s.rays, i), st,
                    [](int, int, float, float, float) {}, image);
            }
            film_add_wave(film, pixel, lit, lit ? s.color_r[i] * inv_spp : 0.0f, lit ? s.color_g[i] * inv_spp : 0.0f,
                lit ? s.color_b[i] * inv_spp : 0.0f);
        }
        int t_next = 0;
        if (lane == 0) t_next = atomicAdd(counter, 1);
        t = stripe_waves + __builtin_amdgcn_readfirstlane(t_next);
    }
}

// Persistent form WITH LANE REFILL (rodent_hip_render_trace_refill): a wave does not wait for the last ray of a 64-ray chunk.
// As soon as `refill_idle` of its lanes are idle it retires their rays (shadow rays: film contribution; abandoned rays: deep
// list), draws that many rays from its stripe's counter (ONE atomic per refill) and starts them in the idle lanes; the rest
// keep stepping.  Bounce and shadow rays are incoherent: their step counts inside a chunk differ by an order of magnitude
// and a chunk runs at a quarter of its lanes (standalone, 8 Mi random segments: closest hit +15 %, any hit +22 %,
// profiles/r03_sweep_refill_big_random.log) -- camera rays are not (the same kernel on 16 Mi primary rays: -18 %), and the
// host knows where they are: the stream is [survivors of the last bounce | rays generated for this launch], so draws that
// start inside [coherent_from, n_primary) wait for the whole wave like a chunk does.
// One index space for both lists: g < P = the closest-hit ray g of `p` (P = n_primary rounded up to whole chunks), g >= P the
// shadow ray g - P of `s`; ticket t of stripe s is index ((t / 2048) * 64 + s) * 2048 + t % 2048 (the same 32-chunk groups as
// k_trace_persist); a wave's first 64 tickets are static.  Which rays share a wave changes, what a ray visits does not.
// Lane state next to the ray: `g` = index in the joint space (low 28 bits; -1 = no ray) with bit kFoundBit = "an accepted triangle"
// (what a shadow ray's film contribution depends on; a ray handed to the deep list sets it too: k_trace_deep decides for it).
// Kept small on purpose: 64 VGPRs is the budget of 8 waves per SIMD, and a spill lands inside the step.
struct RefillLane { RayX ray; int top; lds_int* sp; int g; };
constexpr int kFoundBit = 1 << 29, kIndexMask = (1 << 28) - 1;
// SHADOW_ORDER (RODENT_HIP_SHADOW_ORDER): what a node step does with an any-hit (shadow) ray when both children are hit
// -- 0 = the nearer child first, like a closest-hit ray (the reference: src/render/mapping_gpu.impala:47-80 shares the kernel); 1 (the
// default from round 5 on) = child 0 first, no ordering; 2 = the FARTHER child first (the light's side: a shadow ray runs from the surface
// to the light).  Occlusion does not depend on the order, so films and counts do not (checked: scripts/render_rules_check.py).  Measured on
// config 5's frame (profiles/r05_render_rules_check.txt): 1 = +3.0 ... 4.1 %, 2 = +2.7 ... 3.7 % -- an any-hit ray wants an occluder, not
// the nearest one, and the builder orders a node's children by decreasing reference count (bvh.h:215): child 0 is the bigger subtree.
// joint_fetch with the memory records addressed as ONE wave-uniform base (an SGPR pair) + a 32-bit byte offset per lane (global_load ...
// vaddr32, saddr): (traversal_device.h joint_fetch is the form for two arrays anywhere): the scene's node and triangle arrays lie in one
// allocation less than 4 GiB long -- no 64-bit address per lane, no array bases in VGPRs: six registers fewer around the step.
__device__ __forceinline__ void joint_fetch_off(vf4& q0, vf4& q1, vf4& q2, vi2& ids, int& popped, bool in_lds, unsigned lds_addr,
    gbytes base, unsigned off, unsigned off_ids, lds_int* sp) {
    const unsigned long long lds_mask = __ballot(in_lds);
    const unsigned sp_addr = (unsigned)(size_t)sp;
    unsigned long long save;
    asm volatile("s_mov_b64 %[save], exec\n\t"
                 "s_andn2_b64 exec, exec, %[lm]\n\t"
                 "s_cbranch_execz .Ljoint_c_%=\n\t"
                 "global_load_dwordx4 %[q1], %[o], %[sb] offset:16\n\t"
                 "global_load_dwordx4 %[q0], %[o], %[sb]\n\t"
                 "global_load_dwordx4 %[q2], %[o], %[sb] offset:32\n\t"
                 "global_load_dwordx2 %[ch], %[oc], %[sb]\n"
                 ".Ljoint_c_%=:\n\t"
                 "s_and_b64 exec, %[save], %[lm]\n\t"
                 "s_cbranch_execz .Ljoint_d_%=\n\t"
                 "ds_read_b128 %[q0], %[l]\n\t"
                 "ds_read_b128 %[q1], %[l] offset:16\n\t"
                 "ds_read_b128 %[q2], %[l] offset:32\n\t"
                 "ds_read_b64 %[ch], %[l] offset:48\n"
                 ".Ljoint_d_%=:\n\t"
                 "s_mov_b64 exec, %[save]\n\t"
                 "ds_read_b32 %[pop], %[sp]\n\t"
                 "s_waitcnt vmcnt(0) lgkmcnt(0)"
                 : [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [ch] "=&v"(ids), [pop] "=&v"(popped), [save] "=&s"(save)
                 : [o] "v"(off), [oc] "v"(off_ids), [sb] "s"(base), [l] "v"(lds_addr), [sp] "v"(sp_addr), [lm] "s"(lds_mask)
                 : "memory", "scc");               // (s_andn2_b64 / s_and_b64 write SCC)
}

// The streams arrive as SLABS: one base pointer and the capacity -- array k of a stream is base + k * capacity (carve_primary /
// carve_secondary: 0 id, 1..3 org, 4..6 dir, 7 tmin, 8 tmax; primary 9..13 geom_id, prim_id, t, u, v; secondary 9 prim_id, 10..12 colour).
// As the ABI's structs of 20 + 13 pointers this kernel kept ~45 SGPR pairs alive around its loop, 51 of its SGPRs lived in the lanes of a
// VGPR and came back with v_readlane (VALU instructions) at every refill and every accepted triangle; an array's address is now two SALU
// instructions away from three registers.  The host checks that a stream IS a slab (stream_slab) and sends any other one through
// k_trace_persist.  flags: kHitRecordsAoS (primary).
struct StreamSlab { float* base; int cap; int flags; };
// LAZY_MISS (RODENT_HIP_LAZY_MISS): no miss record when a closest-hit ray starts -- it is stored when the ray retires
// without an accepted triangle (kFoundBit), with the tmax read from the stream again.  In a closed scene nearly every ray finds a triangle
// and the record stored up front was 20 of the ~43 bytes this kernel wrote per ray.
template <int SHADOW_ORDER = 0, bool LAZY_MISS = false>
__global__ __launch_bounds__(kWave * kPersistWaves) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_trace_refill(SceneDev sc, StreamSlab pslab, int n_primary, int coherent_from, StreamSlab sslab, const int* size_ptr, int n_value,
    float* film, float inv_spp,
                    int* deep_count_primary, int* deep_count_secondary, unsigned long long* counters, int* deep_list_primary,
                        int* deep_list_secondary, int* tickets,
                    int idle_bounce, int idle_shadow, int* spill, int* err, unsigned tri_delta) {
    constexpr int kStackInts = kPersistWaves * (kTopStack + 1) * kWave, kGroupRays = 32 * kWave;
    __shared__ __attribute__((aligned(16))) int lds[kStackInts + kPersistTopNodes * 16];
    const int lane = threadIdx.x % kWave, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    lds_int* image = (lds_int*)lds + kStackInts;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    for (int j = threadIdx.x; j < kPersistTopNodes * 4; j += kWave * kPersistWaves)
        reinterpret_cast<__attribute__((address_space(3))) i32x4*>(image)[j] = reinterpret_cast<const i32x4*>(sc.top_image_large)[j];
    const int np = n_primary, ns = sslab.base ? stream_size(size_ptr, n_value) : 0;
    const auto P_ = [&](int k) { return pslab.base + (size_t)k * (size_t)pslab.cap; };
    const auto S_ = [&](int k) { return sslab.base + (size_t)k * (size_t)sslab.cap; };
    const auto stream_ray = [&](const float* base, size_t cap, int i) {
        return make_rayx(base[cap + i], base[2 * cap + i], base[3 * cap + i], base[4 * cap + i], base[5 * cap + i], base[6 * cap + i],
            base[7 * cap + i], base[8 * cap + i]);
    };
    const auto hit_record = [&](unsigned i, int geom, int prim, float t, float u, float v) {               // store_hit_record on the slab
        int* g = reinterpret_cast<int*>(P_(9));
        if (pslab.flags & kHitRecordsAoS) {
            int* rec = g + 5u * i;
            *reinterpret_cast<i32x4_dword_aligned*>(rec) = i32x4_dword_aligned{geom, prim, __float_as_int(t), __float_as_int(u)};
            rec[4] = __float_as_int(v);
        } else { g[i] = geom; reinterpret_cast<int*>(P_(10))[i] = prim; P_(11)[i] = t; P_(12)[i] = u; P_(13)[i] = v; }
    };
    const int P = (np + kWave - 1) / kWave * kWave, total = P + ns;
    const int stripe = blockIdx.x % kTraceStripes, stripe_waves = (gridDim.x / kTraceStripes) * kPersistWaves;
    int* counter = tickets + stripe * kTraceCounterStride;
    const auto index_of = [&](int t) { return ((t / kGroupRays) * kTraceStripes + stripe) * kGroupRays + t % kGroupRays; };
    // wave-uniform; lane l's column starts at wave_stack + l
    lds_int* const wave_stack = (lds_int*)lds + wave * (kTopStack + 1) * kWave;
    // sp >= wave_limit  <=>  the lane's cursor is at entry kTopStack (l < kWave)
    lds_int* const wave_limit = wave_stack + kTopStack * kWave;
    __syncthreads();
    if (np && threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(&counters[0], (unsigned long long)np);
    // the scene's nodes and triangles lie in ONE allocation (rodent_hip_scene_create): one wave-uniform base, 32-bit byte offsets per lane
    // (joint_fetch_off). tri_delta = bytes from node id 0's (fictitious) record to triangle 0, checked by the host (bvh_offsets_ok)
    // together with the 24-bit index range of the multiply below
    typedef const __attribute__((address_space(1))) char* gptr;
    const gptr bvh_base = (gptr)reinterpret_cast<const char*>(sc.nodes - 1);                       // node ids are 1-based

    RefillLane L; L.top = 0; L.g = -1; L.sp = wave_stack + lane;
    // rays that ended since the last refill leave the wave: wave-uniform control flow (film_add_wave shuffles)
    const auto retire = [&]() {
        const bool done = L.g >= 0 && L.top == 0;
        const int i = (L.g & kIndexMask) - P;
        const bool lit = done && i >= 0 && !(L.g & kFoundBit);
        if (__ballot(lit))
            film_add_wave(film, lit ? reinterpret_cast<const int*>(S_(0))[i] : -1, lit, lit ? S_(10)[i] * inv_spp : 0.0f,
                lit ? S_(11)[i] * inv_spp : 0.0f, lit ? S_(12)[i] * inv_spp : 0.0f);
        // (tmax: read again from the stream, the bits the caller gave -- the lane holds the canonical value, which differs for a
        // signalling NaN or a denormal, and the record up front and the reference store what was loaded)
        if (LAZY_MISS && done && i < 0 && !(L.g & kFoundBit)) hit_record((unsigned)L.g, sc.num_materials, -1, P_(8)[L.g], 0.0f, 0.0f);
        if (done) L.g = -1;
    };
    const auto start = [&](int g) {
        RayX ray;
        if (g < P) {
            if (g >= np) return;
            ray = stream_ray(pslab.base, (size_t)pslab.cap, g);
            // the miss record; hits overwrite it
            if (!LAZY_MISS) hit_record((unsigned)g, sc.num_materials, -1, ray.tmax, 0.0f, 0.0f);
        } else {
            const int i = g - P;
            if (i >= ns || reinterpret_cast<const int*>(S_(0))[i] < 0) return;
            ray = stream_ray(sslab.base, (size_t)sslab.cap, i);
        }
        ray.tmin = canonical(ray.tmin); ray.tmax = canonical(ray.tmax);
        L.ray = ray; L.g = g;
        L.sp = wave_stack + lane; *L.sp = 0; L.top = kLdsTag;
    };

    // (a prefetched ticket range per wave -- the atomic of the next refill issued at this one -- was measured: 3 % slower, the reserved
    // rays are missing at the launch's end)
    bool more = true, first_draw = true;
    int need_idle = 0;
    for (;;) {
        const unsigned long long live = __ballot(L.top != 0);
        const int idle = kWave - __popcll(live);
        if (more && idle >= need_idle && idle > 0) {
            retire();
            int first;
            // rank in the stripe, wave-major
            if (first_draw) { first = (wave * ((int)gridDim.x / kTraceStripes) + (int)blockIdx.x / kTraceStripes) * kWave;
                first_draw = false; }
            else {
                int f = 0;
                if (lane == 0) f = atomicAdd(counter, idle);
                first = stripe_waves * kWave + __builtin_amdgcn_readfirstlane(f);
            }
            const int g0 = index_of(first);
            // index_of grows with the ticket: once past the end, always past the end
            more = g0 < total;
            need_idle = (g0 >= coherent_from && g0 < P) ? kWave : (g0 < P ? idle_bounce : idle_shadow);   // camera rays: chunk by chunk
            if (L.top == 0) {
                const int g = index_of(first + __popcll(~live & ((1ull << lane) - 1ull)));
                if (g < total) start(g);
            }
            const unsigned long long shadows = __ballot(L.top != 0 && L.g >= P && !((live >> lane) & 1ull));
            if (lane == 0 && shadows) atomicAdd(&counters[4 + ((first / kWave) & 63)], (unsigned long long)__popcll(shadows));
            continue;
        }
        if (live == 0) { retire(); break; }
        if (L.top != 0) {
            // one step of trace_one (the same visit order, the same arithmetic); any hit / closest hit is a property of the lane here
            const int top = L.top;
            const bool is_node = top > 0;
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            typedef int i32x2 __attribute__((ext_vector_type(2)));
            f32x4 q0, q1, q2;
            i32x2 ch;
            int popped;
            {
                // both kinds of fetch -- LDS image, memory -- and the word under the cursor in flight together (joint_fetch_off,
                // traversal_device.h)
                const unsigned idx = (unsigned)(is_node ? top : ~top), stride = is_node ? (unsigned)sizeof(Node2) : (unsigned)sizeof(Tri1);
                // (idx < 2^24: bvh_offsets_ok; a lane on an image link computes an offset nobody loads)
                const unsigned off = __umul24(idx, stride) + (is_node ? 0u : tri_delta);
                joint_fetch_off(q0, q1, q2, ch, popped, top >= kLdsTag, (unsigned)(size_t)image + (unsigned)(top - kLdsTag), bvh_base, off,
                    off + (is_node ? 48u : 40u), L.sp);
            }
            if (is_node) {
                float te0, te1;
                // -(o * 1/d) is computed here, not carried (make_rayx's product, the same value): three multiplications per node step for
                // three registers -- with them in the lane state the register allocator puts three ray components into scratch and reloads
                // them in every step
                RayX rr = L.ray; rr.iox = -(rr.ox * rr.idx); rr.ioy = -(rr.oy * rr.idy); rr.ioz = -(rr.oz * rr.idz);
                const bool h0 = slab_canonical(rr, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, te0) && ch.x != 0;
                const bool h1 = slab_canonical(rr, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, te1) && ch.y != 0;
                bool c0first = te0 < te1;
                if (SHADOW_ORDER != 0) { const bool shadow = (L.g & kIndexMask) >= P;
                    c0first = shadow ? (SHADOW_ORDER == 1 ? true : te0 > te1) : c0first; }
                const bool both = h0 && h1;
                L.top = both ? (c0first ? ch.x : ch.y) : (h0 ? ch.x : (h1 ? ch.y : popped));
                L.sp[kWave] = c0first ? ch.y : ch.x;
                L.sp += (both ? kWave : 0) - ((h0 || h1) ? 0 : kWave);
                // deeper than the window: the oldest entries move out
                if (both && L.sp >= wave_limit) stack_spill<kTopStack>(L.sp, L.top, wave_limit + lane, spill, kPersistWaves, err);
            } else {
                const int prim_id = __float_as_int(q2.w);
                const float nx = cross_x(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z), ny = cross_y(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z),
                    nz = cross_z(q1.x, q1.y, q1.z, q2.x, q2.y, q2.z);
                float t, u, v;
                const bool any = (L.g & kIndexMask) >= P;
                bool found = false;
                if (intersect_tri(L.ray, q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z, nx, ny, nz, t, u, v)) {
                    if (!any) {
                        unsigned k = (unsigned)L.g & (unsigned)kIndexMask;
                        asm volatile("" : "+v"(k));
                        hit_record(k, __float_as_int(q1.w), prim_id & 0x7FFFFFFF, t, u, v);
                    }
                    L.ray.tmax = t; found = true; L.g |= kFoundBit;
                }
                const bool leave = prim_id < 0, ends = any && found;
                L.top = ends ? 0 : (leave ? popped : top - 1);
                L.sp -= (leave && !ends) ? kWave : 0;
            }
            // popped row 0 while entries are out: they come back
            if (L.top >= kSpillMark) stack_reload<kTopStack>(L.sp, L.top, wave_limit + lane, spill, kPersistWaves);
        }
    }
}

// The rays the one-chunk stream kernels (k_trace_primary / k_trace_secondary: launches below one resident generation of rays) abandoned
// because their stack outgrew the LDS window, traced again from the root with the reference's 64-entry stack ([entry][lane] in LDS).
// kDeepGroups one-wave workgroups behind every stream traversal launch, each taking every kDeepGroups-th batch of 64 rays (one
// wave until round 4: a launch with many deep rays waited for a serial drain); workgroup 0 also resets the persistent kernels' ticket
// counters and the shader's slot counter, and the last workgroup to finish resets the list (`done`: zero between launches).
constexpr int kDeepGroups = 64;
template <bool SECONDARY>
__global__ __launch_bounds__(kWave) void k_trace_deep(SceneDev sc, PrimaryStream p, SecondaryStream s, float* film, float inv_spp,
    int* err, int* deep_count,
                                                      const int* deep_list, int* done, int* tickets, int* zero_word) {
    __shared__ int stack_lds[kStackCap * kWave];
    if (blockIdx.x == 0) {
        // the persistent kernel's 64 ticket counters, ready for its next launch
        if (tickets) tickets[threadIdx.x * kTraceCounterStride] = 0;
        // primary pass: the slot counter of the shader that follows (fused compaction)
        if (zero_word && threadIdx.x == 0) *zero_word = 0;
    }
    const int count = __hip_atomic_load(deep_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    DeepStack st{(lds_int*)stack_lds + threadIdx.x, err};
    for (int k = blockIdx.x * kWave + threadIdx.x; k < count; k += gridDim.x * kWave) {
        const int i = deep_list[k];
        if (SECONDARY) {
            const bool lit = !trace_one<true>(sc.nodes, sc.tris, load_stream_ray(s.rays, i), st, [](int, int, float, float, float) {});
            if (lit) {
                float* px = film + 3 * (size_t)s.rays.id[i];
                unsafeAtomicAdd(px, s.color_r[i] * inv_spp); unsafeAtomicAdd(px + 1, s.color_g[i] * inv_spp);
                unsafeAtomicAdd(px + 2, s.color_b[i] * inv_spp);
            }
        } else {
            trace_primary_ray(sc, p, i, nullptr, &st);
        }
    }
    __syncthreads();
    // every workgroup has read the count before it counts itself done, so the last one may zero it (no deep rays -- the usual case -- :
    // nobody waits for anybody)
    if (threadIdx.x == 0 && count > 0 && atomicAdd(done, 1) == (int)gridDim.x - 1) {
        __hip_atomic_store(deep_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
