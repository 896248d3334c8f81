// render.hip -- wavefront path tracer for MI355X (gfx950) behind the C ABI of include/rodent_render.h.
//
// Replaces (all Impala, compiled by AnyDSL in the reference):
//   src/render/mapping_gpu.impala:223-265  gpu_generate_rays      -> k_generate
//   src/render/mapping_gpu.impala:18-30    gpu_traverse_primary   -> k_trace_stream<false>
//   src/render/mapping_gpu.impala:166-221  gpu_sort_primary       -> k_bin_count / k_bin_scan_blocks / k_bin_scan_bins / k_scatter
//   src/render/mapping_gpu.impala:82-134   gpu_shade              -> k_shade  (one launch, material switch; rays arrive sorted)
//   src/render/mapping_gpu.impala:47-80    gpu_traverse_secondary -> k_trace_stream<true> (+ film accumulation :32-45)
//   src/render/mapping_gpu.impala:267-300  gpu_compact_primary    -> the same binning kernels with key = dead?1:0
//   src/render/mapping_gpu.impala:308-369  gpu_streaming_trace    -> render_rows() host loop
//   src/render/mapping_gpu.impala:371-474  gpu_mega_kernel_trace  -> k_mega / render_rows_mega()
//   src/driver/interface.cpp:359-390,528-563,565-663  stream slabs, film, rodent_* services
//
// CDNA4 notes: SoA streams (one 20 x capacity / 13 x capacity float slab each, driver.impala:24-61) so a
// wavefront's 64 lanes read 64 consecutive words; one wave per workgroup for the traversal kernels
// (per-lane stack window in LDS, deeper entries in scratch); sort and compaction are deterministic
// (per-block histograms + scans, wave ballots for the in-block rank) instead of the reference's global
// atomics, so stream order -- and therefore every test -- is reproducible; the film uses hardware
// fp32 atomic adds.  No MFMA: branchy scalar work.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "device_buffer.h"
#include "rodent_build.h"
#include "rodent_render.h"
#include "shading.h"
#include "traversal_device.h"
#include "traversal_steps.h"

namespace {

using namespace rodent_dev;

constexpr int kBlock = 256;                    // workgroup of the streaming (non-traversal) kernels
constexpr int kShadeBlockDefault = 512;        // ... of the shader (shade_block(): measured 256 / 512 / 1024, profiles/r05_shade_block.txt)
// Rays per workgroup of the binning kernels (k_bin_count, k_scatter).  A workgroup's rays of one bin land in ONE contiguous
// run of the output: with 1024 rays and ten bins a run is ~400 bytes per array instead of ~100 -- whole cache lines instead
// of lines shared with the neighbouring workgroup (which usually runs on another XCD, behind another L2) -- and the per-block
// histogram is a quarter of the size.
constexpr int kBinBlock = 1024;
constexpr int kMaxBins = 1025;                 // mapping_gpu.impala:200,342 (1024 geometries + the "miss" bin)
// Rays per stream.  The reference uses 1 Mi (mapping_gpu.impala:319, sized for ~12 GB boards).  On this chip a 1 Mi-ray
// launch is two rounds of resident waves, all fill and drain; 8 Mi-ray streams render the atrium 25 % faster and the
// Cornell box 9 % faster (round 1), 32 Mi-ray streams another 4.6 % / 4.6 % (profiles/r03_capacity_sweep.txt; 64 Mi: no further gain):
// 7.1 GB of streams out of 288 GB.  Results do not depend on it.  rodent_hip_render_capacity() / RODENT_HIP_STREAM_CAPACITY override it.
constexpr int kDefaultCapacity = 32 * 1024 * 1024;
constexpr long kMaxCapacity = 64l << 20;
static int env_capacity() {
    static const int v = [] { const char* e = getenv("RODENT_HIP_STREAM_CAPACITY"); const long c = e ? atol(e) : 0;
        return c >= 64 && c <= kMaxCapacity ? (int)c : kDefaultCapacity; }();
    return v;
}
// RODENT_HIP_PIXEL_BLOCK: the streaming renderer generates a frame's pixels in blocks of this many pixels squared (default 16; 0: row by
// row, the order of the reference's gpu_generate_rays, mapping_gpu.impala:236-241).  Which pixel a stream slot carries is free -- a
// sample's seed depends on (sample, iter, x, y) only, renderer.impala:28-33 -- and the rays in flight together then start, and bounce, in a
// compact part of the scene instead of along a strip of rows: config 5's frame 1 790 -> 1 771 ms (+1.1 %; 8: +0.6 %, 32 and 64 as 16), ray
// counts identical (profiles/r05_pixel_blocks.txt).
inline int pixel_block() {
    static const int v = [] { const char* e = getenv("RODENT_HIP_PIXEL_BLOCK"); const int b = e ? atoi(e) : 16;
        return b == 8 || b == 16 || b == 32 || b == 64 ? b : 0; }();
    return v;
}
// [0..3] host-visible totals, [4..67] shadow rays (striped), [68..99] megakernel primary rays (striped)
constexpr int kNumCounters = 100;

struct CameraDev { float eye[3], dir[3], up[3], right[3]; float w, h; };

// Stream sizes are either known on the host (passed by value) or live on the device (the valid-hit count
// after sorting): size_ptr != nullptr wins.
__device__ __forceinline__ int stream_size(const int* size_ptr, int n_value) { return size_ptr ? *size_ptr : n_value; }

// ---------------------------------------------------------------------------------------------
// K3: ray generation (mapping_gpu.impala:223-265, renderer.impala:26-40, camera.impala:35-44)
// ---------------------------------------------------------------------------------------------
// on_emit (renderer.impala:26-40): the sample's seed and its camera ray direction
__device__ __forceinline__ v3 emit_sample(const CameraDev& cam, int iter, int film_w, int film_h, int x, int y, int sample,
    uint32_t* rnd_out) {
    uint32_t rnd = fnv_hash(fnv_hash(fnv_hash(fnv_hash(0x811C9DC5u, (uint32_t)sample), (uint32_t)iter), (uint32_t)x), (uint32_t)y);
    const float kx = 2.0f * ((float)x + randf(&rnd)) / (float)film_w - 1.0f;
    const float ky = 1.0f - 2.0f * ((float)y + randf(&rnd)) / (float)film_h;
    *rnd_out = rnd;
    return normalize(add(add(mulf(LD3(cam.right), cam.w * kx), mulf(LD3(cam.up), cam.h * ky)), LD3(cam.dir)));
}

// Pixels of a call: [first_pixel, ...) contiguous (tile_pixels == 0: a row band), or interleaved row tiles -- local pixel q is pixel
// first_pixel + (q / tile_pixels) * stride_pixels + q % tile_pixels (rodent_hip_render_tiles: the film's row tiles dealt round-robin to the
// GPUs).
// MOTION (a moving scene, rodent_render.h): a third draw behind the pixel sample's two is the path's shutter sample u; the stored rnd is
// the state behind it and the depth word holds u's 23 mantissa bits above the depth 0.  k_generate<false> is the kernel as it was.
template <bool MOTION = false>
__global__ __launch_bounds__(kBlock) void k_generate(PrimaryStream p, int first_dst, int first_ray_id, int num_rays, CameraDev cam,
                                                      int iter, int film_w, int film_h, int first_pixel, int spp, int tile_pixels,
                                                          int stride_pixels,
                                                      int block = 0, int band_rows = 0) {
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    if (gid >= num_rays) return;
    const int ray_id = first_ray_id + gid, dst = first_dst + gid;
    const int sample = ray_id % spp, q = ray_id / spp;
    // local: the pixel's index in rows that are contiguous in the film (the call's band, or one of its tiles)
    int tile = 0, local = q;
    if (tile_pixels > 0) { tile = q / tile_pixels; local = q - tile * tile_pixels; }
    // block x block pixels after one another instead of whole rows (pixel_block(), below); band_rows: rows of the band / a tile
    if (block > 0) {
        const int strip = local / (block * film_w), i = local - strip * (block * film_w);
        if ((strip + 1) * block <= band_rows) local =
            (strip * block + (i % (block * block)) / block) * film_w + (i / (block * block)) * block + i % block;
    }
    const int pixel = first_pixel + tile * stride_pixels + local;
    const int y = pixel / film_w, x = pixel - y * film_w;          // the reference uses fast_div (common.impala:19-35): same quotient
    uint32_t rnd;
    const v3 d = emit_sample(cam, iter, film_w, film_h, x, y, sample, &rnd);
    p.rays.id[dst] = pixel;
    p.rays.org_x[dst] = cam.eye[0]; p.rays.org_y[dst] = cam.eye[1]; p.rays.org_z[dst] = cam.eye[2];
    p.rays.dir_x[dst] = d.x; p.rays.dir_y[dst] = d.y; p.rays.dir_z[dst] = d.z;
    p.rays.tmin[dst] = 0.0f; p.rays.tmax[dst] = FLT_MAX_REF;
    int depth_word = 0;
    if constexpr (MOTION) depth_word = (int)(xorshift(&rnd) & 0x7FFFFFu) << RODENT_MOTION_DEPTH_BITS;       // randf's mantissa bits
    p.rnd[dst] = rnd; p.mis[dst] = 0.0f; p.contrib_r[dst] = 1.0f; p.contrib_g[dst] = 1.0f; p.contrib_b[dst] = 1.0f;
    p.depth[dst] = depth_word;
}

// The other stages' device code, one header each, in the order the kernels are emitted.
#include "instance_inverse.h"        // the fp64 inverse and the interpolation a moving scene's kernels take per ray (render_motion.h)
#include "render_trace.h"

__global__ void k_copy_int(const int* src, int* dst) { *dst = *src; }

#include "render_shade.h"
#include "render_mega.h"
#include "render_sort.h"
#include "render_update.h"
#include "render_instanced.h"
#include "render_motion.h"

// ---------------------------------------------------------------------------------------------
// Host side: per-device state (interface.cpp:324-339), stream slabs, the streaming loop
// ---------------------------------------------------------------------------------------------
struct DevScene {
    bool loaded = false;
    int num_nodes = 0, num_bvh_tris = 0, num_vertices = 0;
    // k_trace_refill's addressing of nodes and triangles from one base (rodent_hip_scene_create); 0 = not possible for this scene
    unsigned tri_delta = 0;
    SceneDev dev{};
    std::vector<void*> allocs;
    // what rodent_hip_scene_refit_device needs (rodent_hip_scene_refit_prepare; in `allocs` like every table): the refit's scratch with
    // its info words behind it, the triangle each light is bound to (-1: none), and for smooth normals the vertices' incidence lists
    // (vertex v: corner_tri[corner_first[v] .. corner_first[v + 1]), ascending (triangle, corner))
    char* refit_scratch = nullptr; int32_t* refit_info = nullptr;
    int *light_tri = nullptr, *corner_first = nullptr, *corner_tri = nullptr;
    bool refit_enqueued = false;               // RenderDevice::ev_refit marks the end of the last device refit of THIS scene
    // An instanced scene (rodent_hip_scene_create_instanced): dev.nodes / dev.tris are the packed object hierarchies and dev.lights the
    // world lights; `inst` is what the two instanced kernels take beside `dev`.  Everything below is in `allocs` except the per-ray slot
    // array, which grows with the stream slabs (ensure_ray_slots) and is freed with the scene.
    bool instanced = false;
    InstancedDev inst{};
    RodentInstanceDesc* descs = nullptr; RodentObject* objects = nullptr;
    Node2* tlas_nodes = nullptr; RodentInstance* instances = nullptr; char* tlas_scratch = nullptr; int32_t* tlas_info = nullptr;
    int *slot_of = nullptr, *light_owner = nullptr; int2* bases = nullptr;
    RodentLight *object_lights = nullptr, *world_lights = nullptr;
    int num_instances = 0, num_objects = 0, num_object_lights = 0;
    size_t ray_slot_cap = 0;
    // A MOVING scene (rodent_hip_scene_create_motion) is an instanced one (`instanced` is set: the options in effect, the per-ray slot
    // array and the launchers' branch are shared) whose records are motion records: `motion_descs` / `motion_instances` stand in for
    // `descs` / `instances`, which stay null, and the kernels take motion_dev() instead of `inst`.
    bool motion = false;
    RodentMotionInstanceDesc* motion_descs = nullptr; RodentMotionInstance* motion_instances = nullptr;
    // Host copies of the objects' ranges and of the RodentObject table, and the deforming set D of rodent_hip_scene_deform_prepare: its
    // range table, the forest refit's scratch with its info words behind it, the vertices D's triangles name with their incidence
    // lists (vertex verts[j]: corner_tri[corner_first[j] .. corner_first[j + 1])), its bound lights {object light, triangle}.  In
    // `deform.allocs`, freed with the scene or when the set is replaced.
    std::vector<RodentObjectRange> object_ranges;
    std::vector<RodentObject> object_table;
    struct DeformSet {
        std::vector<void*> allocs;
        RodentRefitRange* ranges = nullptr; char* scratch = nullptr; int32_t* info = nullptr;
        int *verts = nullptr, *corner_first = nullptr, *corner_tri = nullptr; int2* lights = nullptr;
        int num_listed = 0, num_nodes = 0, num_tris = 0, num_verts = 0, num_lights = 0;
        bool smooth = false, enqueued = false;
    } deform;
};

struct RenderDevice {
    bool init = false;
    int dev = 0;
    DevScene scene;
    int spp = 4, max_path_len = 64;
    float shutter[2] = {0.0f, 1.0f};           // a moving scene's paths draw their times in [open, close] (rodent_hip_render_shutter)
    int capacity = 0;                          // rays per stream; 0 = default (env_capacity())
    // 1 = sort hit rays by material before shading (mapping_gpu.impala:166-221), 0 = shade in stream order (default: the shader is ONE
    // table-driven kernel, not a kernel per material, and the sort costs more than the divergence it removes -- 5 ... 22 % of the frame on
    // every scene of profiles/r03_sort_sweep.txt)
    int sort = 0;
    // in effect: 0 = 2-wave traversal workgroups (31-record image), shadow pass on the second stream; 1 = persistent stream traversal
    // kernels (k_trace_persist: 16-wave workgroups, 255-record image, ticket counters); 2 = joint: both passes of a bounce in ONE
    // persistent launch
    int trace_persistent = 0;
    // -1 = per scene (joint for every scene the per-scene mapping rule sends to the streaming loop), 0 / 1 / 2 = the caller's choice
    int trace_persistent_request = -1;
    // render_rows keeps hit records as 20-byte records (store_hit_record); RODENT_HIP_HIT_AOS=0 / rodent_hip_render_hit_records(dev, 0):
    // the ABI's five arrays
    int hit_records_aos = 1;
    // in effect, persistent traversal launches: > 0 = lane refill (k_trace_refill) once that many lanes of a wave are idle (bounce rays /
    // shadow rays); 0 = whole chunks (k_trace_persist)
    int trace_refill = 0, trace_refill_shadow = 0;
    int trace_refill_request[2] = {-1, -1};    // -1 = per scene (resolve_refill), else the caller's thresholds
    // rays from which a lone pass takes the persistent kernels and a pending shadow pass rides in the next closest-hit launch
    // (rodent_hip_render_persist_min_rays; the tests' way to the persistent kernels with a few thousand rays)
    int persist_min_rays = kPersistMinRays;
    const char* trace_kernel = "";             // the main kernel of the newest launch_trace (rodent_hip_render_trace_kernel_name)
    DeviceBuffer<int> tickets[2]; int num_cus = 0;
    // 1 = the stream traversal kernels stage the scene's top-of-tree image in LDS (2-wave workgroups); 0 = every node from memory
    int lds_image = 1;
    // 0 = rays are moved by the sort (copy_primary_ray), then shaded in place; 1 = the sort only computes the permutation and the shader
    // gathers through it
    int fused_sort = 0;
    // megakernel: 1 = shadow ray and next path ray of a lane traced in one loop (k_mega_joint: measured slower), 0 = the reference's
    // sequence of loops (k_mega)
    int mega_joint = 0;
    // the shader writes every continuing ray to its compacted slot: 2 = slots from one atomic per block (default), 1 = from a look-back
    // scan (deterministic stream order; measured slower); 0 = shade in place, then the separate compaction pass (mapping_gpu.impala:267-300
    // as it stands)
    int fused_compact = 2;
    DeviceBuffer<unsigned> scan;               // per-block words of the shader's look-back scan (zero before every launch)
    DeviceBuffer<int> perm;                    // sorted position -> stream index
    int mapping = 0;                           // in effect: 0 = streaming wavefront (mapping_gpu.impala:308-369), 1 = megakernel (:371-474)
    int mapping_request = -1;                  // -1 = chosen per scene (auto_mapping), 0 / 1 = the caller's choice
    float* film = nullptr; int film_w = 0, film_h = 0;
    DeviceBuffer<float> slab[3];                   // first primary, second primary, secondary
    DeviceBuffer<int> tmp;
    // rays handed to k_trace_deep: [0] primary, [1] secondary (may run at the same time)
    DeviceBuffer<int> deep_list[2];
    DeviceBuffer<int> deep_done[2];                // k_trace_deep's workgroup counters (zero between launches)
    // out-of-window stack entries of the persistent traversal launches: one block per resident wave (stack_spill); [1]: the shadow pass on
    // the second stream
    DeviceBuffer<int> spill[2];
    hipStream_t aux = nullptr;                     // shadow-ray traversal runs here, beside the compaction / next primary pass
    hipEvent_t ev_shade = nullptr, ev_sec = nullptr, ev_copy = nullptr;
    hipEvent_t ev_refit = nullptr;                 // recorded behind every rodent_hip_scene_refit_device (DevScene::refit_enqueued)
    int overlap = 1;                               // 0: everything on the caller's stream
    DeviceBuffer<int> hist;
    int* ctl = nullptr;       // [0] primary size, [1] secondary size, [2] error flag, [8..] bin_total, bin_begin, bin_end (kMaxBins each)
    unsigned long long* counters = nullptr;    // [0] primary rays, [1] unused, [2] iterations, [3] generated, [4..67] shadow rays (striped)
    // rodent_hip_render_tiles: its sub-calls after the first ADD to the counters instead of starting them again
    bool counters_continue = false;
    unsigned long long call_iterations = 0, call_generated = 0;
    int* host_pinned = nullptr;
    int32_t create_flags = 0;                  // device flags of the last rodent_hip_scene_create_instanced that failed on them
    // `buf`, about to be ensure()d for n elements: a buffer that has to grow allocates on the current device, so that is made this one
    template <typename T> DeviceBuffer<T>& growing(DeviceBuffer<T>& buf, size_t n) {
        if (buf.count < n) HIP_CHECK(hipSetDevice(dev));
        return buf;
    }
};
RenderDevice g_rdev[16];
std::mutex g_rmutex;
int g_current_dev = 0;
std::vector<float> g_host_film; size_t g_host_w = 0, g_host_h = 0;

// every option of the renderer at its default, or at what its environment variable says (rodent_hip_render_defaults)
// an option's environment variable, if set: clamped to [lo, hi]; a switch (0, 1) is on for every non-zero value
void env_int(const char* name, int lo, int hi, int& field) {
    if (const char* e = getenv(name)) field = (lo == 0 && hi == 1) ? atoi(e) != 0 : std::min(hi, std::max(lo, atoi(e)));
}
void render_defaults(RenderDevice& r) {
    r.hit_records_aos = 1;
    r.sort = 0; r.overlap = 1; r.fused_sort = 0; r.fused_compact = 2; r.mega_joint = 0; r.lds_image = 1; r.trace_persistent_request = -1;
    r.mapping_request = -1; r.capacity = 0; r.trace_refill_request[0] = r.trace_refill_request[1] = -1;
    r.persist_min_rays = kPersistMinRays;
    r.shutter[0] = 0.0f; r.shutter[1] = 1.0f;
    env_int("RODENT_HIP_HIT_AOS", 0, 1, r.hit_records_aos); env_int("RODENT_HIP_SORT", 0, 1, r.sort);
    env_int("RODENT_HIP_OVERLAP", 0, 1, r.overlap); env_int("RODENT_HIP_FUSED_SORT", 0, 1, r.fused_sort);
    env_int("RODENT_HIP_FUSED_COMPACT", 0, 2, r.fused_compact); env_int("RODENT_HIP_LDS_IMAGE", 0, 1, r.lds_image);
    env_int("RODENT_HIP_MEGA_JOINT", 0, 1, r.mega_joint); env_int("RODENT_HIP_TRACE_PERSISTENT", -1, 2, r.trace_persistent_request);
    // "48", "48,32" (bounce rays, shadow rays), "0" = off, "-1" = per scene
    if (const char* e = getenv("RODENT_HIP_TRACE_REFILL")) {
        const char* c = strchr(e, ',');
        const int a = std::min(kWave, std::max(-1, atoi(e))), b = c ? std::min(kWave, std::max(-1, atoi(c + 1))) : a;
        if ((a > 0) != (b > 0) || (a < 0) != (b < 0)) {
            fprintf(stderr, "rodent_hip: RODENT_HIP_TRACE_REFILL=%s: both thresholds must be positive, both 0 (off) or both -1 (per "
            "scene), as for rodent_hip_render_trace_refill\n", e); abort(); }
        if (a > 0 && b > 0) { r.trace_refill_request[0] = a; r.trace_refill_request[1] = b; }
        else r.trace_refill_request[0] = r.trace_refill_request[1] = (a < 0 || b < 0) ? -1 : 0;
    }
    if (const char* m = getenv("RODENT_HIP_MAPPING")) {
        if (!strcmp(m, "mega") || !strcmp(m, "megakernel") || !strcmp(m, "1")) r.mapping_request = 1;
        else if (!strcmp(m, "streaming") || !strcmp(m, "0")) r.mapping_request = 0;
        else if (strcmp(m, "auto") && strcmp(m, "-1")) {
            fprintf(stderr, "rodent_hip: RODENT_HIP_MAPPING must be 'auto', 'streaming' or 'mega'\n"); abort(); }
    }
    r.mapping = r.mapping_request == 1 ? 1 : 0;
    r.trace_persistent = std::max(0, r.trace_persistent_request);
}

// what the next frame does about the sort by material: the per-ray slot array of an instanced scene is not moved by the sort
int sort_in_effect(const RenderDevice& r) { return r.scene.instanced ? 0 : r.sort; }
// ... and about the path length: a moving scene's depth word keeps eight bits for the depth
int path_len_in_effect(const RenderDevice& r) {
    return r.scene.motion ? std::min(r.max_path_len, RODENT_MOTION_DEPTH_MASK) : r.max_path_len;
}
// the ray generation of the scene that is loaded
decltype(&k_generate<false>) generate_kernel(const RenderDevice& r) { return r.scene.motion ? k_generate<true> : k_generate<false>; }
// what the kernels of a moving scene take beside SceneDev: the scene's tables and the shutter as it is now
MotionDev motion_dev(const RenderDevice& r) {
    const DevScene& s = r.scene;
    return MotionDev{s.tlas_nodes, s.motion_instances, s.bases, s.inst.ray_slots, r.shutter[0], r.shutter[1]};
}

RenderDevice& rdev(int dev) {
    if (dev < 0 || dev >= 16) { fprintf(stderr, "rodent_hip: invalid device index %d\n", dev); abort(); }
    std::lock_guard<std::mutex> lock(g_rmutex);
    RenderDevice& r = g_rdev[dev];
    if (!r.init) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || dev >= count) {
            fprintf(stderr, "rodent_hip: no HIP device %d (%d visible)\n", dev, count); abort(); }
        HIP_CHECK(hipSetDevice(dev));
        r.dev = dev;
        HIP_CHECK(hipMalloc(&r.ctl, sizeof(int) * (8 + 6 * kMaxBins)));
        HIP_CHECK(hipMemset(r.ctl, 0, sizeof(int) * (8 + 6 * kMaxBins)));
        HIP_CHECK(hipMalloc(&r.counters, sizeof(unsigned long long) * kNumCounters));
        HIP_CHECK(hipMemset(r.counters, 0, sizeof(unsigned long long) * kNumCounters));
        HIP_CHECK(hipHostMalloc(&r.host_pinned, sizeof(int) * (8 + kMaxBins)));
        render_defaults(r);
        // k_scatter ranks inside 1024-ray blocks with one counter row per wave: 16 x num_bins ints of dynamic LDS, 65 600 bytes at the
        // 1025 bins kMaxBins allows -- more than the 64 KB a launch gets without asking
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_scatter), hipFuncAttributeMaxDynamicSharedMemorySize,
            (int)(sizeof(int) * (kBinBlock / kWave) * kMaxBins)));
        r.init = true;
    }
    return r;
}

inline int round_cap(int size) { return (size & ~31) + 32; }                 // interface.cpp:359-366

// may_fail: an allocation the device has no room for returns nullptr (the slab is gone then) instead of aborting
float* ensure_slab(RenderDevice& r, int which, int size, int multiplier, bool may_fail = false) {
    const size_t n = (size_t)round_cap(size) * multiplier;
    return may_fail ? r.growing(r.slab[which], n).try_ensure(n, 0) : r.growing(r.slab[which], n).ensure(n, 0);
}

void carve_rays(RayStream& rays, float* ptr, size_t cap) {                    // interface.cpp:528-538
    rays.id = (int32_t*)ptr; rays.org_x = ptr + 1 * cap; rays.org_y = ptr + 2 * cap; rays.org_z = ptr + 3 * cap;
    rays.dir_x = ptr + 4 * cap; rays.dir_y = ptr + 5 * cap; rays.dir_z = ptr + 6 * cap; rays.tmin = ptr + 7 * cap;
    rays.tmax = ptr + 8 * cap;
}
void carve_primary(PrimaryStream& p, float* ptr, size_t cap) {               // interface.cpp:540-554
    carve_rays(p.rays, ptr, cap);
    p.geom_id = (int32_t*)ptr + 9 * cap; p.prim_id = (int32_t*)ptr + 10 * cap; p.t = ptr + 11 * cap; p.u = ptr + 12 * cap;
    p.v = ptr + 13 * cap;
    p.rnd = (uint32_t*)ptr + 14 * cap; p.mis = ptr + 15 * cap; p.contrib_r = ptr + 16 * cap; p.contrib_g = ptr + 17 * cap;
    p.contrib_b = ptr + 18 * cap;
    p.depth = (int32_t*)ptr + 19 * cap; p.size = 0; p.pad = 0;
}
void carve_secondary(SecondaryStream& s, float* ptr, size_t cap) {           // interface.cpp:556-563
    carve_rays(s.rays, ptr, cap);
    s.prim_id = (int32_t*)ptr + 9 * cap; s.color_r = ptr + 10 * cap; s.color_g = ptr + 11 * cap; s.color_b = ptr + 12 * cap; s.size = 0;
    s.pad = 0;
}

void ensure_deep(RenderDevice& r, int which, int rays) {
    r.growing(r.deep_list[which], rays).ensure(rays);
    r.deep_done[which].ensure(16, 0);
}
int shadow_order() { static const int v = [] { const char* e = getenv("RODENT_HIP_SHADOW_ORDER");
    return e ? std::min(2, std::max(0, atoi(e))) : 1; }(); return v; }
// 1 (default from round 6 on): films and ray counts identical, frame rates +0.1 ... 0.3 % on atrium / gallery / Cornell box
// (profiles/r06_lazy_miss_render.txt), 20 bytes per closest-hit ray less to write; 0 = the record up front (until round 5).  (Through the
// traversal ABI the same idea LOSES 2 ... 8 %: profiles/r06_lazy_miss_traversal.txt.)
int lazy_miss() { static const int v = [] { const char* e = getenv("RODENT_HIP_LAZY_MISS"); return e ? (atoi(e) != 0) : 1; }(); return v; }
// the k_trace_refill instantiation those two ask for (every shadow order has both forms of the miss record), and its name
struct NamedRefill { decltype(&k_trace_refill<0>) kernel; const char* name; };
NamedRefill pick_trace_refill() {
    static const NamedRefill kRefill[3][2] = {
        {{k_trace_refill<0, false>, "k_trace_refill<0,false>"}, {k_trace_refill<0, true>, "k_trace_refill<0,true>"}},
        {{k_trace_refill<1, false>, "k_trace_refill<1,false>"}, {k_trace_refill<1, true>, "k_trace_refill<1,true>"}},
        {{k_trace_refill<2, false>, "k_trace_refill<2,false>"}, {k_trace_refill<2, true>, "k_trace_refill<2,true>"}}};
    return kRefill[shadow_order()][lazy_miss() ? 1 : 0];
}
// The other kernels of a lone pass: the whole-chunk persistent kernel, the one-chunk kernels (2-wave workgroups with the scene's
// top-of-tree image in LDS / one wave, every node from memory: lds_image) and the follow-up kernel.  (Both passes in one launch:
// k_trace_persist<2>.)
template <typename OneChunk> struct PassKernels {
    decltype(&k_trace_persist<0>) persist; OneChunk image, plain; decltype(&k_trace_deep<false>) deep;
    const char *persist_name, *image_name, *plain_name;
};
static_assert(kTraceWaves == 2 && kSceneTopNodes == 31, "the kernel names below");
const PassKernels<decltype(&k_trace_primary<1, 0>)> kClosestKernels{k_trace_persist<0>, k_trace_primary<kTraceWaves, kSceneTopNodes>,
    k_trace_primary<1, 0>, k_trace_deep<false>, "k_trace_persist<0>", "k_trace_primary<2,31>", "k_trace_primary<1,0>"};
const PassKernels<decltype(&k_trace_secondary<1, 0>)> kShadowKernels{k_trace_persist<1>, k_trace_secondary<kTraceWaves, kSceneTopNodes>,
    k_trace_secondary<1, 0>, k_trace_deep<true>, "k_trace_persist<1>", "k_trace_secondary<2,31>", "k_trace_secondary<1,0>"};
int persistent_grid(RenderDevice& r) {
    if (!r.num_cus) { hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, r.dev)); r.num_cus = prop.multiProcessorCount; }
    return ((r.num_cus * (32 / kPersistWaves) + kTraceStripes - 1) / kTraceStripes) * kTraceStripes;
}
// the spill blocks of a persistent launch on stream `which` (103 MB for the 8192 resident waves of this chip, allocated with the first such
// launch)
int* ensure_spill(RenderDevice& r, int which) {
    const size_t n = (size_t)persistent_grid(r) * kPersistWaves * kSpillWaveInts;
    return r.growing(r.spill[which], n).ensure(n);
}
void ensure_tickets(RenderDevice& r) { for (auto& t : r.tickets) t.ensure(kTraceStripes * kTraceCounterStride, 0); }
// k_trace_refill keeps a ray's index in 28 bits of a lane register (the renderer's own streams hold at most 64 Mi rays each; a caller's
// stage-level streams may be larger: those go through k_trace_persist) A stream as k_trace_refill takes it (StreamSlab): the base and the
// capacity of a stream whose arrays lie `cap` words apart in carve order, or ok = false (a caller's stage-level struct may point anywhere:
// such a stream goes through k_trace_persist).  An empty struct (all null) is the slab {null, 0}.
bool arrays_slab(const void* const* arrays, int count, int flags, StreamSlab& out) {
    float* base = (float*)arrays[0];
    const ptrdiff_t cap = (const float*)arrays[1] - base;
    out = StreamSlab{base, (int)cap, flags};
    if (!base) return true;
    if (cap <= 0 || cap > 0x7FFFFFFF) return false;
    for (int k = 0; k < count; k++) if (arrays[k] != base + (size_t)k * (size_t)cap) return false;
    return true;
}
bool stream_slab(const PrimaryStream& p, StreamSlab& out) {
    const void* const arrays[20] = {p.rays.id, p.rays.org_x, p.rays.org_y, p.rays.org_z, p.rays.dir_x, p.rays.dir_y, p.rays.dir_z,
        p.rays.tmin, p.rays.tmax, p.geom_id, p.prim_id, p.t, p.u, p.v, p.rnd, p.mis, p.contrib_r, p.contrib_g, p.contrib_b, p.depth};
    return arrays_slab(arrays, 20, p.pad & kHitRecordsAoS, out);
}
bool stream_slab(const SecondaryStream& s, StreamSlab& out) {
    const void* const arrays[13] = {s.rays.id, s.rays.org_x, s.rays.org_y, s.rays.org_z, s.rays.dir_x, s.rays.dir_y, s.rays.dir_z,
        s.rays.tmin, s.rays.tmax, s.prim_id, s.color_r, s.color_g, s.color_b};
    return arrays_slab(arrays, 13, 0, out);
}
// Threads per workgroup of the shader = rays per slot request of its fused compaction.  The request is one returning atomic on ONE word
// (the new stream size), and one word serves ~88 atomics per microsecond: at 256 rays per request (until round 5) a full 32 Mi-ray stream
// asks 131 072 times, 77 per microsecond of the shader's 1.7 ms. 512: config 5 +1.4 ... 2.0 %, crown +1.8 %, gallery +0.7 %, the Cornell
// box through the streaming loop +8.6 %; 1024 gives half of that back to its two barriers over sixteen waves
// (profiles/r05_shade_block.txt).  RODENT_HIP_SHADE_BLOCK=256|512|1024.
int shade_block() { static const int v = [] { const char* e = getenv("RODENT_HIP_SHADE_BLOCK");
    const int b = e ? atoi(e) : kShadeBlockDefault; return b == 256 || b == 512 || b == 1024 ? b : kShadeBlockDefault; }(); return v; }
// b: threads per workgroup, 256 / 512 / 1024 (the renderer's own launches pass shade_block())
template <typename... Args> void launch_k_shade(hipStream_t stream, int b, int rays, Args... args) {
    const int blocks = (rays + b - 1) / b;
    if (b == 256) hipLaunchKernelGGL((k_shade<256, false>), dim3(blocks), dim3(256), 0, stream, args...);
    else if (b == 512) hipLaunchKernelGGL((k_shade<512, false>), dim3(blocks), dim3(512), 0, stream, args...);
    else hipLaunchKernelGGL((k_shade<1024, false>), dim3(blocks), dim3(1024), 0, stream, args...);
}
// (Dev: InstancedDev, or MotionDev for a moving scene)
template <typename Dev, typename... Args> void launch_k_shade_instanced(hipStream_t stream, int b, int rays, const Dev& inst,
                                                                        Args... args) {
    const int blocks = (rays + b - 1) / b;
    if (b == 256) hipLaunchKernelGGL((k_shade<256, true, Dev>), dim3(blocks), dim3(256), 0, stream, args..., inst);
    else if (b == 512) hipLaunchKernelGGL((k_shade<512, true, Dev>), dim3(blocks), dim3(512), 0, stream, args..., inst);
    else hipLaunchKernelGGL((k_shade<1024, true, Dev>), dim3(blocks), dim3(1024), 0, stream, args..., inst);
}
// the shader of the scene that is loaded
template <typename... Args> void launch_shader(RenderDevice& r, hipStream_t stream, int b, int rays, Args... args) {
    if (r.scene.motion) launch_k_shade_instanced(stream, b, rays, motion_dev(r), args...);
    else if (r.scene.instanced) launch_k_shade_instanced(stream, b, rays, r.scene.inst, args...);
    else launch_k_shade(stream, b, rays, args...);
}
// The per-ray slot array of an instanced scene: at least n ints, and never fewer than the device's stream slabs hold rays, so that a
// pointer handed out by rodent_hip_scene_instances stays valid while the streams do.  Growing it waits for the device.
void ensure_ray_slots(RenderDevice& r, size_t n) {
    DevScene& s = r.scene;
    n = std::max(n, std::max(std::max(r.slab[0].count, r.slab[1].count) / 20, r.slab[2].count / 13));
    n = std::max<size_t>(n, 64);
    if (n <= s.ray_slot_cap) return;
    HIP_CHECK(hipSetDevice(r.dev));
    if (s.inst.ray_slots) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipFree(s.inst.ray_slots)); }
    s.inst.ray_slots = nullptr; s.ray_slot_cap = 0;
    HIP_CHECK(hipMalloc(&s.inst.ray_slots, sizeof(int32_t) * n));
    HIP_CHECK(hipMemset(s.inst.ray_slots, 0, sizeof(int32_t) * n));
    HIP_CHECK(hipStreamSynchronize(nullptr));               // (the fill does not wait for the host: DeviceBuffer::grow)
    s.ray_slot_cap = n;
}
bool refill_indexable(long long n_primary, long long n_secondary) { return n_primary + kWave + n_secondary <= (long long)kIndexMask; }
// One stream traversal launch -- the main kernel, then the one-wave kernel for the rays it abandoned -- over a closest-hit pass, a shadow
// pass, or BOTH in one persistent launch (the joint form: asked for only with persistent kernels on and n >= persist_min_rays).  A pass
// that is absent is the empty struct.
// coherent_from: the rays [coherent_from, n) were generated for this launch (camera rays), the ones in front of them are what the last
// bounce left; < 0 = the caller does not know (the stage-level hip_traverse_primary): a lone closest-hit pass then takes whole chunks
// through k_trace_persist -- with coherent_from = 0 every draw of k_trace_refill would wait for the whole wave anyway, in the heavier loop
// (ADVICE r3).
// ctl words: [2] error flag, [3] primary deep count, [4] secondary deep count, [5] secondary stream size (copy for the aux stream),
// [6] the shader's slot counter
struct ClosestPass { const PrimaryStream* p = nullptr; int n = 0, coherent_from = 0; };
// (size *size_ptr, or max_n; unoccluded rays add their colour x inv_spp to the film)
struct ShadowPass { const SecondaryStream* s = nullptr; const int* size_ptr = nullptr; int max_n = 0; float inv_spp = 0.0f; };
// An instanced scene: one launch per pass, no follow-up kernel (render_instanced.h).
void launch_trace_instanced(RenderDevice& r, hipStream_t stream, const ClosestPass& c, const ShadowPass& sh) {
    const DevScene& s = r.scene;
    if (s.motion) {                                      // a moving scene: the same two launches over the motion records
        if (c.p) {
            ensure_ray_slots(r, (size_t)c.n);
            r.trace_kernel = "k_trace_instanced_motion<false>";
            hipLaunchKernelGGL(k_trace_instanced_motion<false>, dim3((c.n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev,
                motion_dev(r), *c.p, SecondaryStream{}, (const int*)nullptr, c.n, (float*)nullptr, 0.0f, r.counters, r.ctl + 2, r.ctl + 6);
        }
        if (sh.s) {
            r.trace_kernel = "k_trace_instanced_motion<true>";
            hipLaunchKernelGGL(k_trace_instanced_motion<true>, dim3((sh.max_n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev,
                motion_dev(r), PrimaryStream{}, *sh.s, sh.size_ptr, sh.max_n, r.film, sh.inv_spp, r.counters, r.ctl + 2, (int*)nullptr);
        }
        return;
    }
    if (c.p) {
        ensure_ray_slots(r, (size_t)c.n);
        r.trace_kernel = "k_trace_instanced<false>";
        hipLaunchKernelGGL(k_trace_instanced<false>, dim3((c.n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev, s.inst, *c.p,
            SecondaryStream{}, (const int*)nullptr, c.n, (float*)nullptr, 0.0f, r.counters, r.ctl + 2, r.ctl + 6);
    }
    if (sh.s) {
        r.trace_kernel = "k_trace_instanced<true>";
        hipLaunchKernelGGL(k_trace_instanced<true>, dim3((sh.max_n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev, s.inst,
            PrimaryStream{}, *sh.s, sh.size_ptr, sh.max_n, r.film, sh.inv_spp, r.counters, r.ctl + 2, (int*)nullptr);
    }
}
void launch_trace(RenderDevice& r, hipStream_t stream, const ClosestPass& c, const ShadowPass& sh) {
    if (r.scene.instanced) { launch_trace_instanced(r, stream, c, sh); return; }
    const bool joint = c.p && sh.s;
    const int which = c.p ? 0 : 1;         // ticket array and spill block: [1] = a lone shadow pass (it may run beside a closest-hit one)
    const PrimaryStream p = c.p ? *c.p : PrimaryStream{};
    const SecondaryStream s = sh.s ? *sh.s : SecondaryStream{};
    float* const film = sh.s ? r.film : nullptr;
    if (c.p) ensure_deep(r, 0, c.n);
    if (sh.s) ensure_deep(r, 1, sh.max_n);
    int* tickets = nullptr;
    if (joint || (r.trace_persistent && (c.p ? c.n : sh.max_n) >= r.persist_min_rays)) {
        ensure_tickets(r); tickets = r.tickets[which].ptr;
        StreamSlab ps{nullptr, 0, 0}, ss{nullptr, 0, 0};
        const bool refill = r.trace_refill > 0 && r.scene.tri_delta && (sh.s || c.coherent_from >= 0) && refill_indexable(c.n, sh.max_n)
            && (!c.p || stream_slab(p, ps)) && (!sh.s || stream_slab(s, ss));
        const dim3 grid(persistent_grid(r)), block(kWave * kPersistWaves);
        // what every persistent kernel's argument list ends in (k_trace_refill: with its thresholds `idle...` in front of the spill block)
        const auto with_tail = [&](auto launch, auto... idle) {
            launch(sh.size_ptr, sh.max_n, film, sh.inv_spp, r.ctl + 3, r.ctl + 4, r.counters, r.deep_list[0].ptr, r.deep_list[1].ptr,
                tickets, idle..., ensure_spill(r, which), r.ctl + 2);
        };
        r.trace_kernel = refill ? pick_trace_refill().name : joint ? "k_trace_persist<2>" : c.p ? kClosestKernels.persist_name
            : kShadowKernels.persist_name;
        if (refill) with_tail([&](auto... tail) { hipLaunchKernelGGL(pick_trace_refill().kernel, grid, block, 0, stream, r.scene.dev, ps,
            c.n, c.coherent_from, ss, tail..., r.scene.tri_delta); }, r.trace_refill, r.trace_refill_shadow);
        else with_tail([&](auto... tail) { hipLaunchKernelGGL(joint ? k_trace_persist<2> : c.p ? kClosestKernels.persist
            : kShadowKernels.persist, grid, block, 0, stream, r.scene.dev, p, c.n, s, tail...); });
    } else {
        const int waves = r.lds_image ? kTraceWaves : 1, rays = c.p ? c.n : sh.max_n;
        r.trace_kernel = c.p ? (r.lds_image ? kClosestKernels.image_name : kClosestKernels.plain_name)
            : (r.lds_image ? kShadowKernels.image_name : kShadowKernels.plain_name);
        const dim3 grid((rays + waves * kWave - 1) / (waves * kWave)), block(waves * kWave);
        if (c.p) hipLaunchKernelGGL(r.lds_image ? kClosestKernels.image : kClosestKernels.plain, grid, block, 0, stream, r.scene.dev, p,
            (const int*)nullptr, c.n, r.ctl + 3, r.counters, r.deep_list[0].ptr);
        else hipLaunchKernelGGL(r.lds_image ? kShadowKernels.image : kShadowKernels.plain, grid, block, 0, stream, r.scene.dev, s,
            sh.size_ptr, sh.max_n, film, sh.inv_spp, r.ctl + 4, r.counters, r.deep_list[1].ptr);
    }
    // The follow-up kernels.  (Nothing is abandoned by the persistent kernels any more: behind a joint launch one group is the launch's
    // housekeeping -- ticket counters, the shader's slot counter -- and the shadow pass gets none.)
    if (c.p) hipLaunchKernelGGL(kClosestKernels.deep, dim3(joint ? 1 : kDeepGroups), dim3(kWave), 0, stream, r.scene.dev, p,
        SecondaryStream{}, (float*)nullptr, 0.0f, r.ctl + 2, r.ctl + 3, r.deep_list[0].ptr, r.deep_done[0].ptr, tickets, r.ctl + 6);
    else hipLaunchKernelGGL(kShadowKernels.deep, dim3(kDeepGroups), dim3(kWave), 0, stream, r.scene.dev, PrimaryStream{}, s, film,
        sh.inv_spp, r.ctl + 2, r.ctl + 4, r.deep_list[1].ptr, r.deep_done[1].ptr, tickets, (int*)nullptr);
}

// two sets of bin arrays: set 0 = sort by geometry, set 1 = compaction (the compaction reads its input size from set 0)
int* bin_total(RenderDevice& r, int set) { return r.ctl + 8 + set * 3 * kMaxBins; }
int* bin_begin(RenderDevice& r, int set) { return r.ctl + 8 + set * 3 * kMaxBins + kMaxBins; }
int* bin_end(RenderDevice& r, int set)   { return r.ctl + 8 + set * 3 * kMaxBins + 2 * kMaxBins; }

// Bins `p` (size = *size_ptr if given, else max_n; never more than max_n) into `q`; bins >= drop_from_bin are not copied.
void bin_stream(RenderDevice& r, int set, const PrimaryStream& p, const PrimaryStream& q, const int* size_ptr, int max_n, int mode,
    int num_bins,
                int keep_hit, int drop_from_bin, hipStream_t stream, int copy_interval = 1, int* perm = nullptr) {
    const int blocks = std::max(1, (max_n + kBinBlock - 1) / kBinBlock);
    int* const hist = r.hist.ensure((size_t)num_bins * blocks);
    const size_t lds = sizeof(int) * (kBinBlock / kWave) * num_bins;
    hipLaunchKernelGGL(k_bin_count, dim3(blocks), dim3(kBlock), sizeof(int) * num_bins, stream, p, size_ptr, max_n, mode, num_bins, blocks,
        hist);
    hipLaunchKernelGGL(k_bin_scan_blocks, dim3(num_bins), dim3(kBlock), 0, stream, hist, blocks, bin_total(r, set));
    hipLaunchKernelGGL(k_bin_scan_bins, dim3(1), dim3(1), 0, stream, bin_total(r, set), num_bins, bin_begin(r, set), bin_end(r, set));
    hipLaunchKernelGGL(k_scatter, dim3(blocks), dim3(kBinBlock), lds, stream, p, q, size_ptr, max_n, mode, num_bins, blocks, hist,
        bin_begin(r, set), keep_hit, drop_from_bin, copy_interval, perm);
    HIP_CHECK(hipGetLastError());
}

CameraDev to_cam(const Settings* s) {
    CameraDev c;
    c.eye[0] = s->eye.x; c.eye[1] = s->eye.y; c.eye[2] = s->eye.z; c.dir[0] = s->dir.x; c.dir[1] = s->dir.y; c.dir[2] = s->dir.z;
    c.up[0] = s->up.x; c.up[1] = s->up.y; c.up[2] = s->up.z; c.right[0] = s->right.x; c.right[1] = s->right.y; c.right[2] = s->right.z;
    c.w = s->width; c.h = s->height;
    return c;
}

void require_scene(RenderDevice& r) {
    if (!r.scene.loaded) { fprintf(stderr, "rodent_hip: no scene loaded on device %d (call rodent_hip_scene_create)\n", r.dev); abort(); }
    if (r.scene.dev.num_lights <= 0) { fprintf(stderr, "rodent_hip: the scene has no light source\n"); abort(); }
    if (!r.film) { fprintf(stderr, "rodent_hip: no film (call setup_interface)\n"); abort(); }
}

void ensure_film(RenderDevice& r) {
    if (r.film && r.film_w == (int)g_host_w && r.film_h == (int)g_host_h) return;
    HIP_CHECK(hipSetDevice(r.dev));
    if (r.film) HIP_CHECK(hipFree(r.film));
    r.film_w = (int)g_host_w; r.film_h = (int)g_host_h;
    HIP_CHECK(hipMalloc(&r.film, sizeof(float) * 3 * (size_t)r.film_w * r.film_h));
    HIP_CHECK(hipMemset(r.film, 0, sizeof(float) * 3 * (size_t)r.film_w * r.film_h));
}

// What every call that works on the scene opens with: the device current, its film and scene there, and `stream` behind the last
// rodent_hip_scene_refit_device, whichever stream that took (an event, not a device-wide wait).
RenderDevice& open_scene(RenderDevice& r, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(r.dev)); ensure_film(r); require_scene(r);
    if (r.scene.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    return r;
}

// The head of a frame call on `stream`: open_scene, the first `ctl_words` control words zero (the streaming loop uses eight, the megakernel
// the sizes and the error flag only) and the counters started again, or continued (rodent_hip_render_tiles)
void frame_begin(RenderDevice& r, hipStream_t stream, int ctl_words) {
    open_scene(r, stream);
    HIP_CHECK(hipMemsetAsync(r.ctl, 0, sizeof(int) * ctl_words, stream));
    if (!r.counters_continue) { HIP_CHECK(hipMemsetAsync(r.counters, 0, sizeof(unsigned long long) * kNumCounters, stream));
        r.call_iterations = r.call_generated = 0; }
}
// ... and its tail: the call's iterations and generated rays join the counters, the error flag comes back, the stream is drained
void frame_end(RenderDevice& r, hipStream_t stream, unsigned long long iterations, unsigned long long generated) {
    r.call_iterations += iterations; r.call_generated += generated;
    const unsigned long long host_counts[2] = {r.call_iterations, r.call_generated};
    HIP_CHECK(hipMemcpyAsync(r.counters + 2, host_counts, sizeof(host_counts), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(r.host_pinned + 2, r.ctl + 2, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (r.host_pinned[2]) { fprintf(stderr, "rodent_hip: traversal stack overflow in the renderer\n"); abort(); }
}

// gpu_streaming_trace (mapping_gpu.impala:308-369) for image rows [y0, y1) -- or, with tile_rows > 0, for (y1 - y0) rows that are
// row tiles of tile_rows rows each, the first at row y0, the next stride_rows further down, ... (y1 - y0 a multiple of tile_rows)
void render_rows(RenderDevice& r, const Settings* settings, int iter, int y0, int y1, hipStream_t stream, int tile_rows = 0,
    int stride_rows = 0) {
    frame_begin(r, stream, 8);
    const int sort = sort_in_effect(r);
    const int G = r.scene.dev.num_materials;
    if (G + 1 > kMaxBins) { fprintf(stderr, "rodent_hip: too many geometries (%d)\n", G); abort(); }
    PrimaryStream a, b; SecondaryStream sec;
    // rays per stream: the configured capacity, but no more than this call can ever have in flight (a 256 x 144 frame does not reserve 7
    // GB)
    int kCapacity = (int)std::min<long long>(r.capacity > 0 ? r.capacity : env_capacity(),
        std::max<long long>(64, ((long long)r.spp * r.film_w * std::max(0, y1 - y0) + 63) / 64 * 64));
    // The default capacity (32 Mi rays: 7.1 GB of streams) is a choice of speed, not a need: when the device has no room for it (other
    // tenants, a smaller board) the streams are halved until they fit -- results do not depend on the capacity.  A capacity
    // the caller asked for (rodent_hip_render_capacity) is taken literally: failing to get it aborts with HIP's message.
    for (;;) {
        const bool may_fail = r.capacity <= 0 && kCapacity > (1 << 20);
        if (ensure_slab(r, 0, kCapacity, 20, may_fail) && ensure_slab(r, 1, kCapacity, 20, may_fail)
            && ensure_slab(r, 2, kCapacity, 13, may_fail)) break;
        fprintf(stderr, "rodent_hip: no room for ray streams of %d rays on device %d, trying %d\n", kCapacity, r.dev, kCapacity / 2);
        kCapacity /= 2;
    }
    carve_primary(a, ensure_slab(r, 0, kCapacity, 20), round_cap(kCapacity));
    carve_primary(b, ensure_slab(r, 1, kCapacity, 20), round_cap(kCapacity));
    // hit records as 20-byte records instead of five arrays (store_hit_record) -- unless the sort by material runs: its kernels move and
    // read the arrays
    a.pad = b.pad = (r.hit_records_aos && !sort) ? kHitRecordsAoS : 0;
    carve_secondary(sec, ensure_slab(r, 2, kCapacity, 13), round_cap(kCapacity));
    PrimaryStream* primary = &a; PrimaryStream* other = &b;
    const CameraDev cam = to_cam(settings);
    const float inv_spp = 1.0f / (float)r.spp;
    const long long num_rays = (long long)r.spp * r.film_w * (y1 - y0);
    // ray ids are 32-bit in the stream kernels (as in the reference, mapping_gpu.impala:236-241)
    if (num_rays > 0x7FFFFFFFll) {
        fprintf(stderr, "rodent_hip: spp x width x rows = %lld samples in one call exceeds 2^31 - 1; render fewer rows per call or more "
        "frames of fewer spp\n", num_rays); abort(); }
    const int first_pixel = y0 * r.film_w;
    // pixels are generated block by block where the film allows it (whole blocks across, whole tiles down)
    const int block = pixel_block() > 0 && r.film_w % pixel_block() == 0
        && (tile_rows == 0 || (tile_rows % pixel_block() == 0 && r.film_h % tile_rows == 0)) ? pixel_block() : 0;
    long long id = 0; int size = 0;
    unsigned long long iterations = 0, generated = 0;
    const int* d_valid = bin_end(r, 0) + (G - 1);      // rays that hit something = exclusive end of the last geometry bin (:347-357)
    // Shadow rays are independent of what follows the shader on the primary stream (compaction, regeneration, the next
    // closest-hit pass and sort): they are traced on a second HIP stream and joined again before the next shader run
    // overwrites the secondary stream.  The latency-bound traversal then shares the chip with the HBM-bound stream copies.
    // the shadow pass of an iteration rides in the next iteration's closest-hit launch: one stream
    const bool joint = r.trace_persistent == 2;
    const bool overlap = r.overlap != 0 && !joint;
    ShadowPass pending;                            // joint: the shadow pass that waits for the next closest-hit launch
    if (overlap && !r.aux) {
        HIP_CHECK(hipStreamCreateWithFlags(&r.aux, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&r.ev_shade, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&r.ev_sec, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&r.ev_copy, hipEventDisableTiming));
    }
    ensure_deep(r, 0, kCapacity); ensure_deep(r, 1, kCapacity);       // before the loop: growing them synchronises the device
    r.perm.ensure(round_cap(kCapacity));
    if (r.scene.instanced) ensure_ray_slots(r, (size_t)round_cap(kCapacity));
    const bool fused = r.fused_compact != 0;
    int* d_alive = r.ctl + 6;                            // fused compaction: the shader's last block leaves the new stream size here
    if (fused) r.scan.ensure((kCapacity + kBlock - 1) / kBlock);
    // the shader, either in place (then the compaction pass follows) or compacting into the other stream itself
    const auto shade = [&](const PrimaryStream& from, const PrimaryStream& to, const int* perm, const int* size_ptr, int n_value,
        int unsorted, int blocks) {
        if (fused) {
            if (r.fused_compact != 2) HIP_CHECK(hipMemsetAsync(r.scan.ptr, 0, sizeof(unsigned) * (size_t)blocks, stream));
            // (d_alive was zeroed by the primary pass's follow-up kernel, k_trace_deep<false>)
        }
        launch_shader(r, stream, shade_block(), blocks * kBlock, r.scene.dev, from, to, perm, sec, size_ptr, n_value, r.film, inv_spp,
            path_len_in_effect(r), unsorted,
                       fused ? (r.fused_compact == 2 ? kScanAtomic : r.scan.ptr) : (unsigned*)nullptr, d_alive);
    };
    while (id < num_rays || size > 0) {
        // [0, survivors): what the last bounce left; behind them the rays generated now
        const int survivors = size;
        if (size < kCapacity && id < num_rays) {                                         // regenerate (mapping_gpu.impala:332-336)
            const int n = (int)std::min<long long>(num_rays - id, kCapacity - size);
            hipLaunchKernelGGL(generate_kernel(r), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, *primary, size, (int)id, n, cam, iter,
                               r.film_w, r.film_h, first_pixel, r.spp, tile_rows * r.film_w, stride_rows * r.film_w, block,
                                   tile_rows > 0 ? tile_rows : y1 - y0);
            id += n; size += n; generated += n;
        }
        const int blocks = (size + kBlock - 1) / kBlock;
        // joint: the pending shadow pass rides in this closest-hit launch if that is a persistent one, else it goes in front of it
        const bool ride = pending.s && size >= r.persist_min_rays;
        if (pending.s && !ride) launch_trace(r, stream, {}, pending);
        launch_trace(r, stream, {primary, size, survivors}, ride ? pending : ShadowPass{});
        pending = ShadowPass{};
        // Sort by material (:166-221) or shade in stream order (misses end in the shader); sorted, the stream's size is the count of rays
        // that hit something, on the device
        const int* const size_ptr = sort ? d_valid : nullptr;
        int* const perm = sort && r.fused_sort ? r.perm.ptr : nullptr;
        if (sort) {
            // the aux stream has its copy of the previous valid count
            if (overlap && iterations) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_copy, 0));
            // fused: WITHOUT moving the rays -- the binning kernels only compute the permutation, the shader gathers through it and writes
            // the sorted, shaded stream.  Misses (bin G) are dropped either way (:347-357); tmin / tmax stay behind
            bin_stream(r, 0, *primary, *other, nullptr, size, KEY_GEOM, G + 1, 1, G, stream, 0, perm);
            if (!perm) std::swap(primary, other);
        }
        // the previous shadow rays have been traced
        if (overlap && iterations) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_sec, 0));
        if (perm || fused) { shade(*primary, *other, perm, size_ptr, sort ? 0 : size, !sort, blocks); std::swap(primary, other); }
        else shade(*primary, *primary, nullptr, size_ptr, sort ? 0 : size, !sort, blocks);
        // the shadow pass of this iteration: on the second stream, behind the shader on this one, or (joint) inside the next closest-hit
        // launch
        const int* shadow_size_ptr = size_ptr;
        if (overlap) {
            HIP_CHECK(hipEventRecord(r.ev_shade, stream));
            HIP_CHECK(hipStreamWaitEvent(r.aux, r.ev_shade, 0));
            if (sort) {
                hipLaunchKernelGGL(k_copy_int, dim3(1), dim3(1), 0, r.aux, d_valid, r.ctl + 5);
                HIP_CHECK(hipEventRecord(r.ev_copy, r.aux));
                shadow_size_ptr = r.ctl + 5;
            }
        }
        const ShadowPass shadows{&sec, shadow_size_ptr, size, inv_spp};
        if (joint) pending = shadows;
        else launch_trace(r, overlap ? r.aux : stream, {}, shadows);
        if (overlap) HIP_CHECK(hipEventRecord(r.ev_sec, r.aux));
        if (!fused) bin_stream(r, 1, *primary, *other, size_ptr, size, KEY_ALIVE, 2, 0, 1, stream);           // compaction (:267-300)
        if (!fused) std::swap(primary, other);
        HIP_CHECK(hipMemcpyAsync(r.host_pinned, fused ? d_alive : bin_end(r, 1), sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        size = r.host_pinned[0];
        iterations++;
    }
    // joint: the last iteration's shadow rays
    if (pending.s) launch_trace(r, stream, {}, pending);
    if (overlap && iterations) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_sec, 0));           // the last shadow rays belong to this call
    frame_end(r, stream, iterations, generated);
}

// gpu_mega_kernel_trace (mapping_gpu.impala:371-474) for image rows [y0, y1)
void render_rows_mega(RenderDevice& r, const Settings* settings, int iter, int y0, int y1, hipStream_t stream) {
    frame_begin(r, stream, 3);
    int ilog2_spp = 0; while ((2 << ilog2_spp) <= r.spp) ilog2_spp++;                 // common.impala ilog2
    const int log2_tile = std::max(0, (10 - ilog2_spp) / 2);                          // tiles of ~2^10 samples (:374-377)
    const int tile = 1 << log2_tile;
    const dim3 grid((r.film_w + tile - 1) >> log2_tile, (y1 - y0 + tile - 1) >> log2_tile);
    int* err = r.ctl + 2;
    if (y1 > y0) {
        if (r.mega_joint) hipLaunchKernelGGL(k_mega_joint, grid, dim3(kWave), 0, stream, r.scene.dev, to_cam(settings), r.film, r.film_w,
            r.film_h, y0, y1, iter, r.spp,
                                             r.max_path_len, log2_tile, 1.0f / (float)r.spp, err, r.counters);
        else hipLaunchKernelGGL(k_mega<true>, grid, dim3(kWave), 0, stream, r.scene.dev, to_cam(settings), r.film, r.film_w, r.film_h, y0,
            y1, iter, r.spp,
                                r.max_path_len, log2_tile, 1.0f / (float)r.spp, err, r.counters);
    }
    HIP_CHECK(hipGetLastError());
    frame_end(r, stream, 1ull, (unsigned long long)r.spp * r.film_w * (unsigned long long)(y1 - y0));
}

void render_rows_any(RenderDevice& r, const Settings* settings, int iter, int y0, int y1, hipStream_t stream) {
    if (r.mapping == 1) render_rows_mega(r, settings, iter, y0, y1, stream);
    else render_rows(r, settings, iter, y0, y1, stream);
}

// Which mapping renders a scene when the caller leaves the choice to the library (rodent_hip_render_mapping(dev, -1), the
// default).  What separates the two on this chip is whether the hierarchy stays in the caches next to the CUs: then a path's
// traversal steps cost little, the streaming loop's per-bounce stream traffic (sort + shade + regenerate, ~500 bytes per
// ray and bounce) is the frame, and the megakernel -- which keeps a path in registers -- wins (Cornell box, 22 nodes:
// 3.2 against 2.2 Gsamples/s); once traversal dominates, the streaming loop's coherent, sorted wavefronts win (atrium,
// 142 444 nodes: 0.74 against 0.59).  Measured in between (profiles/r03_mapping_sweep.txt: the atrium with every 2nd ... 512th
// face, 76 494 ... 306 nodes): the streaming loop wins all of them, by 5 % at 306 nodes and by 40-50 % from 5 000 nodes on;
// only hierarchies of a few dozen nodes (the whole tree inside the traversal kernels' LDS image) go to the megakernel.
int auto_mega_max_nodes() {
    static const int v = [] { const char* e = getenv("RODENT_HIP_AUTO_MEGA_MAX_NODES"); return e ? atoi(e) : 128; }();
    return v;
}
int resolve_mapping(const RenderDevice& r) {
    if (r.scene.instanced) return 0;                   // the instanced kernels are stream kernels
    if (r.mapping_request >= 0) return r.mapping_request;
    return r.scene.loaded && r.scene.num_nodes <= auto_mega_max_nodes() ? 1 : 0;
}
// The stream traversal launches of the streaming loop when the caller leaves the choice to the library: the joint persistent launch
// for every hierarchy above the megakernel's size class (+3 ... +9 % on the atrium at 306 ... 142 444 nodes, profiles/r03_joint_sweep.txt),
// the 2-wave kernels with the shadow pass on a second stream for a tree of a few dozen nodes (Cornell box: joint -5 %).
int resolve_trace(const RenderDevice& r) {
    if (r.scene.instanced) return 0;
    if (r.trace_persistent_request >= 0) return r.trace_persistent_request;
    return r.scene.loaded && r.scene.num_nodes > auto_mega_max_nodes() ? 2 : 0;
}
// Lane refill in those launches when the caller leaves it to the library: on for hierarchies of 16 Ki nodes and more.  What it buys is the
// spread of the rays' step counts inside a wave (a bounce or shadow ray of the atrium takes between 3 and 150 steps); in a small tree
// every ray is short and the refill's own cost (one atomic, eight loads and a reciprocal per started ray, three more multiplications
// per node step) is not paid back -- profiles/r03_refill_sweep.txt: +8 % at 142 444 nodes, +16 % at 76 494, +8 % at 19 862, +1 % at 9 870,
// -4 ... -11 % from 4 951 nodes down.
constexpr int kRefillMinNodes = 16384, kRefillIdleLanes = 40;
void resolve_refill(RenderDevice& r) {
    if (r.scene.instanced) { r.trace_refill = r.trace_refill_shadow = 0; return; }
    if (r.trace_refill_request[0] >= 0) { r.trace_refill = r.trace_refill_request[0]; r.trace_refill_shadow = r.trace_refill_request[1];
        return; }
    r.trace_refill = r.trace_refill_shadow = r.scene.loaded && r.scene.num_nodes >= kRefillMinNodes ? kRefillIdleLanes : 0;
}

template <typename T> T* upload(DevScene& s, const T* host, size_t count) {
    T* d = nullptr;
    HIP_CHECK(hipMalloc(&d, std::max<size_t>(sizeof(T) * count, 16)));
    if (count) HIP_CHECK(hipMemcpy(d, host, sizeof(T) * count, hipMemcpyHostToDevice));
    s.allocs.push_back(d);
    return d;
}

// host-side stream slabs of rodent_cpu_get_*_stream: per thread, like the reference's (interface.cpp:341-342,507-508)
thread_local std::vector<float> t_cpu_primary, t_cpu_secondary;

} // namespace

void rodent_services_cleanup();                                              // services.hip

extern "C" {

void rodent_hip_set_device(int32_t dev) { rdev(dev); g_current_dev = dev; }

void rodent_hip_scene_destroy(int32_t dev) {
    RenderDevice& r = rdev(dev);
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());
    for (void* p : r.scene.allocs) HIP_CHECK(hipFree(p));
    for (void* p : r.scene.deform.allocs) HIP_CHECK(hipFree(p));
    if (r.scene.inst.ray_slots) HIP_CHECK(hipFree(r.scene.inst.ray_slots));
    r.scene = DevScene();
}

} // extern "C"

namespace {

// Top-of-tree image of the stream traversal kernels (record layout: traversal_device.h build_top_image), `capacity` records of 16 words:
// breadth first from the root; a child that got a slot is a link (kLdsTag + byte offset of its record), the others keep their ids.
std::vector<int32_t> build_image(const Node2* nodes, int capacity) {
    std::vector<int32_t> image((size_t)capacity * 16, 0), slots{1};
    for (size_t k = 0; k < slots.size(); k++) {
        const Node2& nd = nodes[slots[k] - 1];
        int32_t* rec = image.data() + 16 * k;
        memcpy(rec, nd.bounds, 12 * sizeof(float));
        for (int j = 0; j < 2; j++) {
            const int32_t c = nd.child[j];
            rec[12 + j] = c;
            if (c > 0 && (int)slots.size() < capacity) { rec[12 + j] = kLdsTag + (int32_t)slots.size() * (int32_t)sizeof(Node2);
                slots.push_back(c); }
        }
        rec[14] = slots[k];
    }
    return image;
}

// SceneDev::tri_shade records (12 floats per triangle): the face normal, then the three corners' vertex normals, gathered.
std::vector<float> tri_shade(const float* face_normals, const float* normals, const int32_t* indices, int32_t num_tris) {
    std::vector<float> rec(12 * (size_t)num_tris);
    for (int32_t t = 0; t < num_tris; t++) {
        float* o = rec.data() + 12 * (size_t)t;
        const float* fn = face_normals + 4 * (size_t)t;
        o[0] = fn[0]; o[1] = fn[1]; o[2] = fn[2];
        for (int k = 0; k < 3; k++) {
            const float* n = normals + 4 * (size_t)indices[4 * (size_t)t + k];
            o[3 + 3 * k] = n[0]; o[4 + 3 * k] = n[1]; o[5 + 3 * k] = n[2];
        }
    }
    return rec;
}

// SceneDev::tri_shade and ::tri_tex of the tables in `d` (host), uploaded into `s`
void upload_shading_records(DevScene& s, const RodentSceneDesc* d, bool textured) {
    // SceneDev::tri_shade: per triangle face normal + its three vertex normals, gathered (RODENT_HIP_TRI_SHADE=0: not built, the shader
    // goes through indices -> normals)
    {
        static const bool on = [] { const char* e = getenv("RODENT_HIP_TRI_SHADE"); return !e || atoi(e) != 0; }();
        s.dev.tri_shade = nullptr;
        if (on && d->num_tris > 0) {
            const std::vector<float> rec = tri_shade(d->face_normals, d->normals, d->indices, d->num_tris);
            s.dev.tri_shade = reinterpret_cast<const float4*>(upload(s, rec.data(), rec.size()));
        }
        s.dev.tri_tex = nullptr;
        // SceneDev::tri_tex: the corners' texture coordinates, for resolve_material
        if (on && textured && d->num_tris > 0) {
            std::vector<float> tc(6 * (size_t)d->num_tris);
            for (int32_t t = 0; t < d->num_tris; t++)
                for (int k = 0; k < 3; k++) {
                    const float* c = d->texcoords + 4 * (size_t)d->indices[4 * (size_t)t + k];
                    tc[6 * (size_t)t + 2 * k] = c[0]; tc[6 * (size_t)t + 2 * k + 1] = c[1];
                }
            s.dev.tri_tex = upload(s, tc.data(), tc.size());
        }
    }
}

// rodent_hip_scene_create and rodent_hip_scene_create_device_bvh(_opt / _split): build = NULL uploads the caller's hierarchy
// (desc->nodes / tris), build options build one on the device from the vertices and indices just uploaded (bvh_build.hip; with
// `split`, over pre-split references) and takes a host copy of it; from there on both are the same code: checks, LDS images, per-scene
// rules.
void scene_create(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* build, const RodentSplitOptions* split = nullptr,
                  const RodentPlocOptions* ploc = nullptr) {
    RenderDevice& r = rdev(dev);
    rodent_hip_scene_destroy(dev);
    HIP_CHECK(hipSetDevice(dev));
    DevScene& s = r.scene;
    s.dev.vertices = upload(s, d->vertices, 4 * (size_t)d->num_vertices);
    s.dev.normals = upload(s, d->normals, 4 * (size_t)d->num_vertices);
    s.dev.face_normals = upload(s, d->face_normals, 4 * (size_t)d->num_tris);
    s.dev.indices = upload(s, d->indices, 4 * (size_t)d->num_tris);
    RodentSceneDesc built_desc;                 // d with the device-built hierarchy (host copy) in place of the caller's
    std::vector<Node2> built_nodes;
    std::vector<Tri1> built_tris;
    {   // nodes and triangles in ONE allocation: k_trace_refill addresses both from one base with 32-bit offsets (joint_fetch_off)
        // (a device-built hierarchy: room for the builder's max(1, refs - 1) nodes, then its refs triangles; the builder's scratch and
        // info words.  Unsplit: refs = n, 4 info words, info[4] keeps n)
        int32_t refs = d->num_tris, info_words = RODENT_BUILD_INFO_WORDS;
        int64_t scratch_bytes = build ? rodent_hip_build_opt_scratch_bytes(d->num_tris, build) : 0;
        if (split) {
            refs = (int32_t)rodent_hip_build_split_max_refs(d->num_tris, split);
            scratch_bytes = rodent_hip_build_split_scratch_bytes(d->num_tris, build, split);
            info_words = RODENT_BUILD_SPLIT_INFO_WORDS;
        }
        if (ploc) {                                      // the PLOC topology stage, with or without the split front: 8 info words
            scratch_bytes = rodent_hip_build_ploc_scratch_bytes(d->num_tris, build, split, ploc);
            info_words = RODENT_BUILD_SPLIT_INFO_WORDS;
        }
        const size_t node_bytes = sizeof(Node2) * (size_t)(build ? std::max(1, refs - 1) : d->num_nodes);
        const size_t tri_bytes = sizeof(Tri1) * (size_t)(build ? refs : d->num_bvh_tris);
        char* bvh = nullptr;
        HIP_CHECK(hipMalloc(&bvh, std::max<size_t>(node_bytes + tri_bytes, 16)));
        s.allocs.push_back(bvh);
        s.dev.nodes = reinterpret_cast<const Node2*>(bvh);
        s.dev.tris = reinterpret_cast<const Tri1*>(bvh + node_bytes);
        if (build) {
            char* scratch = nullptr;
            int32_t info[RODENT_BUILD_SPLIT_INFO_WORDS] = {0, 0, 0, 0, d->num_tris, 0, 0, 0};
            const size_t info_bytes = 4 * (size_t)info_words;
            HIP_CHECK(hipMalloc(&scratch, (size_t)std::max<int64_t>(scratch_bytes, 0) + info_bytes));
            int32_t* info_dev = reinterpret_cast<int32_t*>(scratch + std::max<int64_t>(scratch_bytes, 0));
            Node2* out_nodes = reinterpret_cast<Node2*>(bvh);
            Tri1* out_tris = reinterpret_cast<Tri1*>(bvh + node_bytes);
            const int32_t rc = ploc
                ? rodent_hip_build_bvh2_tri1_ploc(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, split, ploc,
                                                  out_nodes, out_tris, scratch, info_dev, nullptr)
                : split
                ? rodent_hip_build_bvh2_tri1_split(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, split,
                                                   out_nodes, out_tris, scratch, info_dev, nullptr)
                : rodent_hip_build_bvh2_tri1_opt(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, out_nodes,
                                                 out_tris, scratch, info_dev, nullptr);
            if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH build refused (%d)\n", rc); abort(); }
            HIP_CHECK(hipMemcpy(info, info_dev, info_bytes, hipMemcpyDeviceToHost));
            HIP_CHECK(hipFree(scratch));
            if (info[2]) { fprintf(stderr, "rodent_hip: invalid scene: device BVH build flagged the mesh (%d)\n", info[2]); abort(); }
            built_nodes.resize(info[0]);
            built_tris.resize(info[4]);                  // the references (= num_tris unsplit)
            HIP_CHECK(hipMemcpy(built_nodes.data(), bvh, sizeof(Node2) * built_nodes.size(), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(built_tris.data(), bvh + node_bytes, sizeof(Tri1) * built_tris.size(), hipMemcpyDeviceToHost));
            built_desc = *d;
            built_desc.nodes = built_nodes.data(); built_desc.num_nodes = info[0];
            built_desc.tris = built_tris.data(); built_desc.num_bvh_tris = info[4];
            d = &built_desc;
        } else {
            if (node_bytes) HIP_CHECK(hipMemcpy(bvh, d->nodes, node_bytes, hipMemcpyHostToDevice));
            if (tri_bytes) HIP_CHECK(hipMemcpy(bvh + node_bytes, d->tris, tri_bytes, hipMemcpyHostToDevice));
        }
        // tri_delta: bytes from the record a node id of 0 would have to triangle 0; 0 = not addressable this way (offsets beyond 32 bits,
        // or an index beyond the 24-bit multiply)
        const unsigned long long delta = sizeof(Node2) + node_bytes, end = delta + tri_bytes;
        s.tri_delta = (end < (1ull << 32) && d->num_nodes < (1 << 24) - 1 && d->num_bvh_tris < (1 << 24)) ? (unsigned)delta : 0u;
    }
    s.dev.materials = upload(s, d->materials, (size_t)d->num_materials);
    s.dev.lights = upload(s, d->lights, (size_t)d->num_lights);
    s.dev.light_ids = upload(s, d->light_ids, (size_t)d->num_tris);
    const bool textured = d->num_textures > 0;
    if (textured && (!d->texcoords || !d->textures || !d->texels)) {
        fprintf(stderr, "rodent_hip: scene with textures but without texture data\n"); abort(); }
    s.dev.texcoords = upload(s, d->texcoords, textured ? 4 * (size_t)d->num_vertices : 0);
    s.dev.textures = upload(s, d->textures, textured ? (size_t)d->num_textures : 0);
    s.dev.texels = upload(s, d->texels, textured ? (size_t)d->num_texels : 0);
    for (int32_t k = 0; k < d->num_materials; k++)
        if (d->materials[k].tex_kd < 0 || d->materials[k].tex_kd > d->num_textures || d->materials[k].tex_ks < 0
            || d->materials[k].tex_ks > d->num_textures) {
            fprintf(stderr, "rodent_hip: material %d refers to a texture that does not exist\n", k); abort();
        }
    // every index the kernels follow, checked once on the host tables (a corrupt scene must not become an out-of-bounds read in k_shade /
    // trace_one)
    auto invalid = [](const char* what) { fprintf(stderr, "rodent_hip: invalid scene: %s\n", what); abort(); };
    if (d->num_vertices <= 0 || d->num_tris <= 0 || d->num_nodes <= 0 || d->num_bvh_tris <= 0 || d->num_materials <= 0
        || d->num_lights < 0) invalid("empty table");
    for (int32_t t = 0; t < d->num_tris; t++) {
        for (int k = 0; k < 3; k++) if ((uint32_t)d->indices[4 * t + k] >= (uint32_t)d->num_vertices) invalid("vertex index out of range");
        if ((uint32_t)d->indices[4 * t + 3] >= (uint32_t)d->num_materials) invalid("material index out of range");
        if (d->light_ids[t] < 0 || (d->light_ids[t] > 0 && d->light_ids[t] >= d->num_lights)) invalid("light id out of range");
        // an emitter's triangles are looked up in the light table by the shader (on_hit: sc.lights[light_ids[prim]]): the entry must exist
        if (d->materials[d->indices[4 * t + 3]].emissive
            && d->light_ids[t] >= d->num_lights) invalid("emissive triangle without an entry in the light table");
    }
    for (int32_t k = 0; k < d->num_nodes; k++)
        for (int j = 0; j < 2; j++) {
            const int32_t c = d->nodes[k].child[j];
            if ((c > 0 && c > d->num_nodes) || (c < 0 && ~c >= d->num_bvh_tris)) invalid("BVH child id out of range");
        }
    if (d->tris[d->num_bvh_tris - 1].prim_id >= 0) invalid("the last BVH triangle lacks the end-of-leaf bit");
    for (int32_t k = 0; k < d->num_bvh_tris; k++)
        if ((d->tris[k].prim_id & 0x7FFFFFFF) >= d->num_tris
            || (uint32_t)d->tris[k].geom_id
            >= (uint32_t)d->num_materials) invalid("BVH triangle refers to a primitive or material that does not exist");
    for (int32_t k = 0; k < d->num_textures; k++)
        if (d->textures[k].width <= 0 || d->textures[k].height <= 0
            || (uint64_t)d->textures[k].offset + (uint64_t)d->textures[k].width * (uint64_t)d->textures[k].height
            > d->num_texels) invalid("texture outside the texel pool");
    s.dev.num_tris = d->num_tris; s.dev.num_materials = d->num_materials; s.dev.num_lights = d->num_lights;
    // top-of-tree images of the stream traversal kernels (build_image)
    for (const int capacity : {kSceneTopNodes, kPersistTopNodes}) {
        const std::vector<int32_t> image = build_image(d->nodes, capacity);
        (capacity == kSceneTopNodes ? s.dev.top_image : s.dev.top_image_large) =
            reinterpret_cast<const int4*>(upload(s, image.data(), image.size()));
    }
    upload_shading_records(s, d, textured);
    s.num_nodes = d->num_nodes;
    s.num_bvh_tris = d->num_bvh_tris;
    s.num_vertices = d->num_vertices;
    s.loaded = true;
    r.mapping = resolve_mapping(r);
    r.trace_persistent = resolve_trace(r);
    resolve_refill(r);
}

// rodent_hip_scene_refit_prepare: one-time and synchronous.  The tables it reads back (indices, light ids, materials) never change under
// a refit, so the lists it builds on the host hold for the scene's life.
void refit_prepare(RenderDevice& r, bool smooth_normals) {
    DevScene& s = r.scene;
    HIP_CHECK(hipSetDevice(r.dev));
    if (!r.ev_refit) HIP_CHECK(hipEventCreateWithFlags(&r.ev_refit, hipEventDisableTiming));
    const size_t nv = (size_t)s.num_vertices, nt = (size_t)s.dev.num_tris;
    std::vector<int32_t> indices;
    if (!s.refit_info || (smooth_normals && !s.corner_first)) {
        indices.resize(4 * nt);
        HIP_CHECK(hipMemcpy(indices.data(), s.dev.indices, sizeof(int32_t) * indices.size(), hipMemcpyDeviceToHost));
    }
    if (!s.refit_info) {
        const int64_t scratch_bytes = std::max<int64_t>(rodent_hip_refit_scratch_bytes(s.num_nodes, s.num_bvh_tris), 0);
        HIP_CHECK(hipMalloc(&s.refit_scratch, (size_t)scratch_bytes + 4 * RODENT_BUILD_INFO_WORDS));
        s.allocs.push_back(s.refit_scratch);
        int32_t* const info = reinterpret_cast<int32_t*>(s.refit_scratch + scratch_bytes);
        HIP_CHECK(hipMemset(info, 0, 4 * RODENT_BUILD_INFO_WORDS));
        // light k: the lowest emissive triangle whose light id is k
        std::vector<int32_t> light_ids(nt);
        std::vector<RodentMaterial> materials((size_t)s.dev.num_materials);
        HIP_CHECK(hipMemcpy(light_ids.data(), s.dev.light_ids, sizeof(int32_t) * nt, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(materials.data(), s.dev.materials, sizeof(RodentMaterial) * materials.size(), hipMemcpyDeviceToHost));
        std::vector<int> light_tri((size_t)s.dev.num_lights, -1);
        for (size_t t = 0; t < nt; t++) {
            const int32_t k = light_ids[t];
            if (materials[indices[4 * t + 3]].emissive && k >= 0 && k < s.dev.num_lights && light_tri[k] < 0) light_tri[k] = (int)t;
        }
        s.light_tri = upload(s, light_tri.data(), light_tri.size());
        s.refit_info = info;
    }
    if (smooth_normals && !s.corner_first) {
        std::vector<int> first(nv + 1, 0), tri(3 * nt);
        for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) first[(size_t)indices[4 * t + k] + 1]++;
        for (size_t v = 0; v < nv; v++) first[v + 1] += first[v];
        std::vector<int> next(first.begin(), first.end() - 1);
        for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) tri[next[indices[4 * t + k]]++] = (int)t;
        s.corner_tri = upload(s, tri.data(), tri.size());
        s.corner_first = upload(s, first.data(), first.size());
    }
}

DevScene& loaded_scene(int32_t dev, const char* entry) {
    DevScene& s = rdev(dev).scene;
    if (!s.loaded) {
        fprintf(stderr, "rodent_hip: %s: no scene loaded on device %d (call rodent_hip_scene_create)\n", entry, dev); abort(); }
    return s;
}
// the refit entries: an instanced scene has no single hierarchy to refit (its instances move with rodent_hip_scene_set_transforms)
DevScene& flat_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (s.instanced) { fprintf(stderr, "rodent_hip: %s: the scene on device %d is instanced (move its instances with "
        "rodent_hip_scene_set_transforms)\n", entry, dev); abort(); }
    return s;
}
// (the static-instance entries: a moving scene is "no instanced scene" to them)
DevScene& instanced_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (!s.instanced || s.motion) {
        fprintf(stderr, "rodent_hip: %s: the scene on device %d is not instanced (rodent_hip_scene_create_instanced)\n", entry, dev);
        abort(); }
    return s;
}
DevScene& motion_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (!s.motion) { fprintf(stderr, "rodent_hip: %s: the scene on device %d has no moving instances (rodent_hip_scene_create_motion)\n",
        entry, dev); abort(); }
    return s;
}

} // namespace

extern "C" {

void rodent_hip_scene_create(int32_t dev, const RodentSceneDesc* d) { scene_create(dev, d, nullptr); }

void rodent_hip_scene_create_device_bvh(int32_t dev, const RodentSceneDesc* d, int32_t max_leaf) {
    const RodentBuildOptions opt{max_leaf, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    rodent_hip_scene_create_device_bvh_opt(dev, d, &opt);
}

void rodent_hip_scene_create_device_bvh_opt(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt) {
    if (!opt || rodent_hip_build_opt_scratch_bytes(1, opt) < 0 || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || d->num_vertices < 1 || d->nodes || d->tris || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh: invalid arguments (max_leaf 1 ... 8, treelet passes 0 ... 3, "
                        "costs in (0, 1e6], 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt);
}

void rodent_hip_scene_create_device_bvh_split(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt,
                                              const RodentSplitOptions* split) {
    if (!opt || !split || rodent_hip_build_split_scratch_bytes(1, opt, split) < 0 || d->num_tris < 1
        || d->num_tris > RODENT_BUILD_MAX_TRIS || d->num_vertices < 1 || d->nodes || d->tris || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh_split: invalid arguments (max_leaf 1 ... 8, treelet passes "
                        "0 ... 3, costs in (0, 1e6], split budget 0 ... 4, max_pieces 1 ... 64, 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt, split);
}

void rodent_hip_scene_create_device_bvh_ploc(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt,
                                             const RodentSplitOptions* split, const RodentPlocOptions* ploc) {
    if (!opt || !ploc || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || rodent_hip_build_ploc_scratch_bytes(d->num_tris, opt, split, ploc) < 0 || d->num_vertices < 1 || d->nodes || d->tris
        || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh_ploc: invalid arguments (max_leaf 1 ... 8, treelet passes "
                        "0 ... 3, costs in (0, 1e6], split budget 0 ... 4, max_pieces 1 ... 64, PLOC radius 1 ... 64, depth limit 0 or "
                        "ceil(log2 references) ... 56 and 56 with treelet passes, wide iterations -1 ... 255, 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt, split, ploc);
}

void rodent_hip_scene_refit(int32_t dev, const float* vertices, const float* normals, const float* face_normals,
                            const RodentLight* lights) {
    RenderDevice& r = rdev(dev);
    DevScene& s = r.scene;
    if (!s.loaded) { fprintf(stderr, "rodent_hip: no scene loaded on device %d (call rodent_hip_scene_create)\n", dev); abort(); }
    flat_scene(dev, "rodent_hip_scene_refit");
    if (!vertices || !normals || !face_normals || (s.dev.num_lights > 0 && !lights)) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_refit: a NULL table\n"); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());                   // no frame still reads the tables that are overwritten
    const size_t nv = (size_t)s.num_vertices, nt = (size_t)s.dev.num_tris;
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.vertices), vertices, sizeof(float) * 4 * nv, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.normals), normals, sizeof(float) * 4 * nv, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.face_normals), face_normals, sizeof(float) * 4 * nt, hipMemcpyHostToDevice));
    if (s.dev.num_lights > 0)
        HIP_CHECK(hipMemcpy(const_cast<RodentLight*>(s.dev.lights), lights, sizeof(RodentLight) * (size_t)s.dev.num_lights,
                            hipMemcpyHostToDevice));
    // the hierarchy, in place: rodent_hip_scene_bvh's pointers stay valid
    Node2* nodes = const_cast<Node2*>(s.dev.nodes);
    Tri1* tris = const_cast<Tri1*>(s.dev.tris);
    const int64_t scratch_bytes = rodent_hip_refit_scratch_bytes(s.num_nodes, s.num_bvh_tris);
    char* scratch = nullptr;
    int32_t info[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipMalloc(&scratch, (size_t)std::max<int64_t>(scratch_bytes, 0) + sizeof(info)));
    int32_t* info_dev = reinterpret_cast<int32_t*>(scratch + std::max<int64_t>(scratch_bytes, 0));
    const int32_t rc = rodent_hip_refit_bvh2_tri1(dev, s.dev.vertices, s.num_vertices, s.dev.indices, s.dev.num_tris, nodes, s.num_nodes,
                                                  tris, s.num_bvh_tris, scratch, info_dev, nullptr);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH refit refused (%d)\n", rc); abort(); }
    HIP_CHECK(hipMemcpy(info, info_dev, sizeof(info), hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(scratch));
    if (info[2] || info[0] != s.num_nodes) {
        fprintf(stderr, "rodent_hip: invalid scene: device BVH refit flagged the mesh or the hierarchy (flags %d, %d of %d nodes)\n",
                info[2], info[0], s.num_nodes); abort(); }
    // what scene_create derives from positions or bounds, into its existing allocations: both LDS images and the tri_shade records
    std::vector<Node2> host_nodes((size_t)s.num_nodes);
    HIP_CHECK(hipMemcpy(host_nodes.data(), nodes, sizeof(Node2) * host_nodes.size(), hipMemcpyDeviceToHost));
    for (const int capacity : {kSceneTopNodes, kPersistTopNodes}) {
        const std::vector<int32_t> image = build_image(host_nodes.data(), capacity);
        const int4* dst = capacity == kSceneTopNodes ? s.dev.top_image : s.dev.top_image_large;
        HIP_CHECK(hipMemcpy(const_cast<int4*>(dst), image.data(), sizeof(int32_t) * image.size(), hipMemcpyHostToDevice));
    }
    if (s.dev.tri_shade) {
        std::vector<int32_t> indices(4 * nt);
        HIP_CHECK(hipMemcpy(indices.data(), s.dev.indices, sizeof(int32_t) * indices.size(), hipMemcpyDeviceToHost));
        const std::vector<float> rec = tri_shade(face_normals, normals, indices.data(), s.dev.num_tris);
        HIP_CHECK(hipMemcpy(const_cast<float4*>(s.dev.tri_shade), rec.data(), sizeof(float) * rec.size(), hipMemcpyHostToDevice));
    }
}

void rodent_hip_scene_refit_prepare(int32_t dev, int32_t smooth_normals) {
    flat_scene(dev, "rodent_hip_scene_refit_prepare");
    refit_prepare(rdev(dev), smooth_normals != 0);
}

void rodent_hip_scene_refit_device(int32_t dev, const float* vertices_dev, const float* normals_dev, void* stream_) {
    DevScene& s = flat_scene(dev, "rodent_hip_scene_refit_device");
    RenderDevice& r = rdev(dev);
    if (!vertices_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_refit_device: NULL vertices\n"); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    if (!s.refit_info || (!normals_dev && !s.corner_first)) refit_prepare(r, !normals_dev);
    hipStream_t stream = (hipStream_t)stream_;
    // Behind the last device refit, whichever stream it took.  Frames need no such wait: a frame call returns when its rows are in the
    // film (frame_end), so none is in flight; the next one waits for ev_refit (open_scene).
    if (s.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    const int nv = s.num_vertices, nt = s.dev.num_tris, nl = s.dev.num_lights;
    float4* const vertices = reinterpret_cast<float4*>(const_cast<float*>(s.dev.vertices));
    float4* const normals = reinterpret_cast<float4*>(const_cast<float*>(s.dev.normals));
    float4* const face_normals = reinterpret_cast<float4*>(const_cast<float*>(s.dev.face_normals));
    const int4* const indices = reinterpret_cast<const int4*>(s.dev.indices);
    if (vertices_dev != s.dev.vertices)
        HIP_CHECK(hipMemcpyAsync(vertices, vertices_dev, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToDevice, stream));
    if (normals_dev && normals_dev != s.dev.normals)
        HIP_CHECK(hipMemcpyAsync(normals, normals_dev, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToDevice, stream));
    const auto blocks = [](int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); };
    hipLaunchKernelGGL(k_face_normals, blocks(nt), dim3(kBlock), 0, stream, vertices, indices, nt, face_normals);
    if (nl > 0) hipLaunchKernelGGL(k_light_records, blocks(nl), dim3(kBlock), 0, stream, vertices, indices, s.light_tri, nl,
                                   const_cast<RodentLight*>(s.dev.lights));
    if (!normals_dev) hipLaunchKernelGGL(k_smooth_normals, blocks(nv), dim3(kBlock), 0, stream, face_normals, s.corner_first,
                                         s.corner_tri, nv, normals);
    // the hierarchy, in place: rodent_hip_scene_bvh's pointers stay valid
    const int32_t rc = rodent_hip_refit_bvh2_tri1(dev, s.dev.vertices, nv, s.dev.indices, nt, const_cast<Node2*>(s.dev.nodes), s.num_nodes,
                                                  const_cast<Tri1*>(s.dev.tris), s.num_bvh_tris, s.refit_scratch, s.refit_info, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH refit refused (%d)\n", rc); abort(); }
    hipLaunchKernelGGL(k_scene_images, dim3(2), dim3(kWave), 0, stream, s.dev.nodes, const_cast<int4*>(s.dev.top_image),
                       const_cast<int4*>(s.dev.top_image_large));
    if (s.dev.tri_shade) hipLaunchKernelGGL(k_tri_shade, blocks(nt), dim3(kBlock), 0, stream, face_normals, normals, indices, nt,
                                            const_cast<float4*>(s.dev.tri_shade));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(r.ev_refit, stream));
    s.refit_enqueued = true;
}

int32_t rodent_hip_scene_refit_status(int32_t dev, int32_t* info) {
    DevScene& s = flat_scene(dev, "rodent_hip_scene_refit_status");
    int32_t words[RODENT_BUILD_INFO_WORDS] = {s.num_nodes, s.num_bvh_tris, 0, 0};      // before the first refit: a sound one's words
    if (s.refit_enqueued) {
        HIP_CHECK(hipSetDevice(dev));
        HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
        HIP_CHECK(hipMemcpy(words, s.refit_info, sizeof(words), hipMemcpyDeviceToHost));
    }
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    return words[2] | (words[0] != s.num_nodes ? (int32_t)0x80000000u : 0);
}

void rodent_hip_scene_tables(int32_t dev, RodentSceneTables* out) {
    const DevScene& s = loaded_scene(dev, "rodent_hip_scene_tables");
    if (!out) return;
    *out = RodentSceneTables{const_cast<float*>(s.dev.vertices), const_cast<float*>(s.dev.normals), const_cast<float*>(s.dev.face_normals),
        const_cast<RodentLight*>(s.dev.lights), reinterpret_cast<float*>(const_cast<float4*>(s.dev.tri_shade)),
        reinterpret_cast<int32_t*>(const_cast<int4*>(s.dev.top_image)),
        reinterpret_cast<int32_t*>(const_cast<int4*>(s.dev.top_image_large)),
        s.num_vertices, s.dev.num_tris, s.dev.num_lights, kSceneTopNodes, kPersistTopNodes};
}

void rodent_hip_scene_bvh(int32_t dev, const Node2** nodes, const Tri1** tris, int32_t* num_nodes, int32_t* num_tris) {
    RenderDevice& r = rdev(dev);
    if (!r.scene.loaded) { fprintf(stderr, "rodent_hip: no scene loaded on device %d (call rodent_hip_scene_create)\n", dev); abort(); }
    *nodes = r.scene.dev.nodes; *tris = r.scene.dev.tris;
    *num_nodes = r.scene.num_nodes; *num_tris = r.scene.num_bvh_tris;
}

// The tables an instanced scene derives from its matrices, enqueued on `stream`: the TLAS and the instance array, slot_of, the world
// lights (rodent_hip_scene_create_instanced, rodent_hip_scene_set_transforms).  Returns rodent_hip_build_tlas's status.
// A moving scene: rodent_hip_build_motion_tlas and the motion forms of the two kernels (the world lights from M0).
static int32_t derive_instanced(int32_t dev, DevScene& s, hipStream_t stream) {
    const auto blocks = [](int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); };
    if (s.motion) {
        const int32_t rc = rodent_hip_build_motion_tlas(dev, s.dev.nodes, s.objects, s.num_objects, s.motion_descs, s.num_instances, 1,
                                                        s.tlas_nodes, s.motion_instances, s.tlas_scratch, s.tlas_info, stream);
        if (rc != RODENT_BUILD_OK) return rc;
        hipLaunchKernelGGL(k_motion_slot_of, blocks(s.num_instances), dim3(kBlock), 0, stream, s.motion_instances, s.num_instances,
                           s.slot_of);
        hipLaunchKernelGGL(k_motion_world_lights, blocks(s.dev.num_lights), dim3(kBlock), 0, stream, s.motion_descs, s.light_owner,
                           s.bases, s.object_lights, s.dev.num_lights, s.world_lights);
        HIP_CHECK(hipGetLastError());
        return rc;
    }
    const int32_t rc = rodent_hip_build_tlas(dev, s.dev.nodes, s.objects, s.num_objects, s.descs, s.num_instances, 1, s.tlas_nodes,
                                             s.instances, s.tlas_scratch, s.tlas_info, stream);
    if (rc != RODENT_BUILD_OK) return rc;
    hipLaunchKernelGGL(k_slot_of, blocks(s.num_instances), dim3(kBlock), 0, stream, s.instances, s.num_instances, s.slot_of);
    hipLaunchKernelGGL(k_world_lights, blocks(s.dev.num_lights), dim3(kBlock), 0, stream, s.descs, s.instances, s.slot_of, s.light_owner,
                       s.bases, s.object_lights, s.dev.num_lights, s.world_lights);
    HIP_CHECK(hipGetLastError());
    return rc;
}

} // extern "C"

// rodent_hip_scene_create_instanced (Desc = RodentInstanceDesc) and rodent_hip_scene_create_motion (RodentMotionInstanceDesc): one
// creation; what differs is the record types, the top-level builder behind derive_instanced and the moving scene's one more refusal.
template <typename Desc>
static int32_t create_instanced_scene(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                                      const Desc* instances, int32_t num_instances, const RodentBuildOptions* opt_) {
    constexpr bool kMotion = std::is_same<Desc, RodentMotionInstanceDesc>::value;
    const RodentBuildOptions default_opt{2, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    const RodentBuildOptions* opt = opt_ ? opt_ : &default_opt;
    // ---- the refusals: all on the host tables, before anything is enqueued or the current scene touched ----
    if (!d || !objects || !instances || num_objects < 1 || num_instances < 1 || num_instances > RODENT_TLAS_MAX_INSTANCES) return
        RODENT_SCENE_ERR_COUNTS;
    const bool textured = d->num_textures > 0;
    if (d->nodes || d->tris || d->num_nodes || d->num_bvh_tris || !d->vertices || !d->normals || !d->face_normals || !d->indices
        || !d->materials || !d->light_ids || d->num_vertices < 1 || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || d->num_materials < 1 || d->num_lights < 0 || (d->num_lights > 0 && !d->lights) || d->num_textures < 0
        || (textured && (!d->texcoords || !d->textures || !d->texels))) return RODENT_SCENE_ERR_COUNTS;
    if (rodent_hip_build_opt_scratch_bytes(1, opt) < 0) return RODENT_SCENE_ERR_OPTIONS;
    {
        int64_t tri = 0, light = 0;
        for (int32_t o = 0; o < num_objects; o++) {
            const RodentObjectRange& r = objects[o];
            if (r.first_tri != tri || r.num_tris < 1 || r.first_light != light || r.num_lights < 0) return RODENT_SCENE_ERR_RANGES;
            tri += r.num_tris; light += r.num_lights;
            if (tri > d->num_tris || light > d->num_lights) return RODENT_SCENE_ERR_RANGES;
        }
        if (tri != d->num_tris || light != d->num_lights) return RODENT_SCENE_ERR_RANGES;
    }
    for (int32_t k = 0; k < d->num_materials; k++)
        if (d->materials[k].tex_kd < 0 || d->materials[k].tex_kd > d->num_textures || d->materials[k].tex_ks < 0
            || d->materials[k].tex_ks > d->num_textures) return RODENT_SCENE_ERR_TABLE;
    for (int32_t k = 0; k < d->num_textures; k++)
        if (d->textures[k].width <= 0 || d->textures[k].height <= 0
            || (uint64_t)d->textures[k].offset + (uint64_t)d->textures[k].width * (uint64_t)d->textures[k].height > d->num_texels)
            return RODENT_SCENE_ERR_TABLE;
    for (int32_t o = 0; o < num_objects; o++) {
        const RodentObjectRange& r = objects[o];
        for (int32_t t = r.first_tri; t < r.first_tri + r.num_tris; t++) {
            for (int k = 0; k < 3; k++)
                if ((uint32_t)d->indices[4 * (size_t)t + k] >= (uint32_t)d->num_vertices) return RODENT_SCENE_ERR_TABLE;
            if ((uint32_t)d->indices[4 * (size_t)t + 3] >= (uint32_t)d->num_materials) return RODENT_SCENE_ERR_TABLE;
            // an emitter's triangles are looked up in the light table by the shader: the entry must exist, and be the object's own
            if (d->materials[d->indices[4 * (size_t)t + 3]].emissive
                && (d->light_ids[t] < r.first_light || d->light_ids[t] >= r.first_light + r.num_lights)) return RODENT_SCENE_ERR_LIGHT;
        }
    }
    int64_t world_lights = 0;
    for (int32_t k = 0; k < num_instances; k++) {
        if (instances[k].object < 0 || instances[k].object >= num_objects) return RODENT_SCENE_ERR_OBJECT;
        world_lights += objects[instances[k].object].num_lights;
    }
    if (world_lights < 1) return RODENT_SCENE_ERR_NO_LIGHT;
    if (world_lights > 0x7FFFFFFF) return RODENT_SCENE_ERR_COUNTS;
    if constexpr (kMotion)                               // lights stay static: an emitter's two keys are equal byte for byte
        for (int32_t k = 0; k < num_instances; k++)
            if (objects[instances[k].object].num_lights > 0
                && std::memcmp(instances[k].object_to_world0, instances[k].object_to_world1, sizeof(float) * 12) != 0)
                return RODENT_SCENE_ERR_MOVING_LIGHT;

    // ---- from here on the device's scene is the new one, or none ----
    RenderDevice& r = rdev(dev);
    rodent_hip_scene_destroy(dev);
    HIP_CHECK(hipSetDevice(dev));
    r.create_flags = 0;
    DevScene& s = r.scene;
    s.dev.vertices = upload(s, d->vertices, 4 * (size_t)d->num_vertices);
    s.dev.normals = upload(s, d->normals, 4 * (size_t)d->num_vertices);
    s.dev.face_normals = upload(s, d->face_normals, 4 * (size_t)d->num_tris);
    s.dev.indices = upload(s, d->indices, 4 * (size_t)d->num_tris);
    s.dev.materials = upload(s, d->materials, (size_t)d->num_materials);
    s.dev.light_ids = upload(s, d->light_ids, (size_t)d->num_tris);
    s.dev.texcoords = upload(s, d->texcoords, textured ? 4 * (size_t)d->num_vertices : 0);
    s.dev.textures = upload(s, d->textures, textured ? (size_t)d->num_textures : 0);
    s.dev.texels = upload(s, d->texels, textured ? (size_t)d->num_texels : 0);
    s.object_lights = upload(s, d->lights, (size_t)d->num_lights);
    const auto fail = [&](int32_t flags) { rodent_hip_scene_destroy(dev); r.create_flags = flags; return RODENT_SCENE_ERR_DEVICE; };
    // every object's hierarchy, built into a block of its own (its node count is known only afterwards), then packed
    std::vector<RodentObject> table((size_t)num_objects);
    std::vector<char*> built((size_t)num_objects, nullptr);
    const auto free_built = [&] { for (char* b : built) if (b) HIP_CHECK(hipFree(b)); };
    int64_t total_nodes = 0;
    // Without treelet passes: ALL objects by one rodent_hip_build_objects call in pack mode (one launch list whatever their number)
    // into a temporary block; the table, the per-object info words and the call's come back in one copy.
    std::vector<RodentRefitRange> plan((size_t)num_objects);
    char* forest = nullptr;                              // nodes (room for max(1, n - 1) each), then, 256-byte aligned, the triangles
    size_t forest_tris = 0;
    int64_t forest_scratch = -1;
    if (opt->treelet_passes == 0) {
        std::vector<int32_t> ids((size_t)num_objects), first((size_t)num_objects), count((size_t)num_objects);
        for (int32_t o = 0; o < num_objects; o++) { ids[o] = o; first[o] = objects[o].first_tri; count[o] = objects[o].num_tris; }
        int32_t totals[2] = {};
        forest_scratch = rodent_hip_build_objects_plan(ids.data(), first.data(), count.data(), num_objects, plan.data(), totals);
    }
    if (forest_scratch >= 0) {
        size_t room = 0;
        for (int32_t o = 0; o < num_objects; o++) room += (size_t)std::max(1, objects[o].num_tris - 1);
        forest_tris = (sizeof(Node2) * room + 255) / 256 * 256;
        const size_t range_bytes = (sizeof(RodentRefitRange) * (size_t)num_objects + 255) / 256 * 256;
        const size_t result_words = 8 * (size_t)num_objects + RODENT_BUILD_INFO_WORDS;    // table, object info, info
        char* work = nullptr;                            // scratch, the range table, the results
        HIP_CHECK(hipMalloc(&forest, forest_tris + sizeof(Tri1) * (size_t)d->num_tris));
        HIP_CHECK(hipMalloc(&work, (size_t)forest_scratch + range_bytes + 4 * result_words));
        RodentRefitRange* ranges_dev = reinterpret_cast<RodentRefitRange*>(work + forest_scratch);
        RodentObject* table_dev = reinterpret_cast<RodentObject*>(work + forest_scratch + range_bytes);
        int32_t* object_info_dev = reinterpret_cast<int32_t*>(table_dev + num_objects);
        int32_t* info_dev = object_info_dev + 4 * (size_t)num_objects;
        HIP_CHECK(hipMemcpy(ranges_dev, plan.data(), sizeof(RodentRefitRange) * (size_t)num_objects, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(table_dev, 0, 4 * result_words));
        const int32_t rc = rodent_hip_build_objects(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, opt->max_leaf,
            RODENT_BUILD_OBJECTS_PACK, reinterpret_cast<Node2*>(forest), reinterpret_cast<Tri1*>(forest + forest_tris), table_dev,
            num_objects, ranges_dev, num_objects, d->num_tris, work, object_info_dev, info_dev, nullptr);
        std::vector<int32_t> result(result_words, 0);
        if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(result.data(), table_dev, 4 * result_words, hipMemcpyDeviceToHost));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(work));
        const int32_t* object_info = result.data() + 4 * (size_t)num_objects;
        int32_t bad = rc;
        for (int32_t o = 0; o < num_objects && !bad; o++) {      // the first flagged object in object order, as the loop reports it
            const int32_t nodes_o = object_info[4 * o], n = objects[o].num_tris;
            bad = object_info[4 * o + 2] ? object_info[4 * o + 2] : nodes_o < 1 || nodes_o > std::max(1, n - 1) ? (int32_t)0x80000000u : 0;
        }
        if (!bad) bad = object_info[4 * (size_t)num_objects + 2];
        if (bad) { HIP_CHECK(hipFree(forest)); return fail(bad); }
        for (int32_t o = 0; o < num_objects; o++) {
            std::memcpy(&table[o], result.data() + 4 * (size_t)o, sizeof(RodentObject));
            total_nodes += table[o].num_nodes;
        }
    }
    for (int32_t o = 0; o < num_objects && !forest; o++) {
        const int32_t n = objects[o].num_tris;
        const size_t node_bytes = sizeof(Node2) * (size_t)std::max(1, n - 1), tri_bytes = sizeof(Tri1) * (size_t)n;
        const int64_t scratch_bytes = std::max<int64_t>(rodent_hip_build_opt_scratch_bytes(n, opt), 0);
        char* scratch = nullptr;
        HIP_CHECK(hipMalloc(&built[o], node_bytes + tri_bytes));
        HIP_CHECK(hipMalloc(&scratch, (size_t)scratch_bytes + 4 * RODENT_BUILD_INFO_WORDS));
        int32_t* info_dev = reinterpret_cast<int32_t*>(scratch + scratch_bytes);
        int32_t info[RODENT_BUILD_INFO_WORDS] = {};
        const int32_t rc = rodent_hip_build_bvh2_tri1_opt(dev, s.dev.vertices, d->num_vertices,
            s.dev.indices + 4 * (size_t)objects[o].first_tri, n, opt, reinterpret_cast<Node2*>(built[o]),
            reinterpret_cast<Tri1*>(built[o] + node_bytes), scratch, info_dev, nullptr);
        if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(info, info_dev, sizeof(info), hipMemcpyDeviceToHost));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(scratch));
        if (rc != RODENT_BUILD_OK || info[2] || info[0] < 1 || info[0] > std::max(1, n - 1)) {
            free_built();
            return fail(rc != RODENT_BUILD_OK ? rc : info[2] ? info[2] : (int32_t)0x80000000u);
        }
        table[o] = RodentObject{(int32_t)total_nodes, objects[o].first_tri, info[0], n};
        total_nodes += info[0];
    }
    {   // one allocation: all nodes, then, 256-byte aligned, all triangles (instances.pack_objects)
        const size_t node_bytes = sizeof(Node2) * (size_t)total_nodes, tri_start = (node_bytes + 255) / 256 * 256;
        char* bvh = nullptr;
        HIP_CHECK(hipMalloc(&bvh, tri_start + sizeof(Tri1) * (size_t)d->num_tris));
        s.allocs.push_back(bvh);
        if (forest) {                                            // packed tight already: the nodes, then the triangles
            HIP_CHECK(hipMemcpy(bvh, forest, node_bytes, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(bvh + tri_start, forest + forest_tris, sizeof(Tri1) * (size_t)d->num_tris, hipMemcpyDeviceToDevice));
        }
        for (int32_t o = 0; o < num_objects && !forest; o++) {
            const size_t from_tris = sizeof(Node2) * (size_t)std::max(1, objects[o].num_tris - 1);
            HIP_CHECK(hipMemcpy(bvh + sizeof(Node2) * (size_t)table[o].node_offset, built[o], sizeof(Node2) * (size_t)table[o].num_nodes,
                                hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(bvh + tri_start + sizeof(Tri1) * (size_t)table[o].tri_offset, built[o] + from_tris,
                                sizeof(Tri1) * (size_t)table[o].num_tris, hipMemcpyDeviceToDevice));
        }
        HIP_CHECK(hipDeviceSynchronize());
        free_built();
        if (forest) HIP_CHECK(hipFree(forest));
        s.dev.nodes = reinterpret_cast<const Node2*>(bvh);
        s.dev.tris = reinterpret_cast<const Tri1*>(bvh + tri_start);
    }
    s.objects = upload(s, table.data(), table.size());
    s.object_table = table;
    s.object_ranges.assign(objects, objects + num_objects);
    // descriptors (ids = indices), bases and light owners: fixed for the scene's life
    std::vector<Desc> descs(instances, instances + num_instances);
    std::vector<int2> bases((size_t)num_instances);
    std::vector<int> owner((size_t)world_lights);
    int32_t light_base = 0;
    for (int32_t k = 0; k < num_instances; k++) {
        descs[k].instance_id = k;
        for (int32_t& word : descs[k].pad) word = 0;
        const RodentObjectRange& o = objects[descs[k].object];
        bases[k] = make_int2(o.first_tri, light_base - o.first_light);
        for (int32_t j = 0; j < o.num_lights; j++) owner[(size_t)light_base + j] = k;
        light_base += o.num_lights;
    }
    s.motion = kMotion;
    if constexpr (kMotion) s.motion_descs = upload(s, descs.data(), descs.size());
    else s.descs = upload(s, descs.data(), descs.size());
    s.bases = upload(s, bases.data(), bases.size());
    s.light_owner = upload(s, owner.data(), owner.size());
    const auto device_block = [&](size_t bytes) { char* p = nullptr; HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
        HIP_CHECK(hipMemset(p, 0, std::max<size_t>(bytes, 16))); s.allocs.push_back(p); return p; };
    s.tlas_nodes = reinterpret_cast<Node2*>(device_block(sizeof(Node2) * (size_t)std::max(1, num_instances - 1)));
    if constexpr (kMotion)
        s.motion_instances = reinterpret_cast<RodentMotionInstance*>(device_block(sizeof(RodentMotionInstance) * (size_t)num_instances));
    else s.instances = reinterpret_cast<RodentInstance*>(device_block(sizeof(RodentInstance) * (size_t)num_instances));
    s.slot_of = reinterpret_cast<int*>(device_block(sizeof(int) * (size_t)num_instances));
    s.world_lights = reinterpret_cast<RodentLight*>(device_block(sizeof(RodentLight) * (size_t)world_lights));
    s.tlas_scratch = device_block((size_t)std::max<int64_t>(
        kMotion ? rodent_hip_motion_tlas_scratch_bytes(num_instances) : rodent_hip_tlas_scratch_bytes(num_instances), 0));
    s.tlas_info = reinterpret_cast<int32_t*>(device_block(4 * RODENT_BUILD_INFO_WORDS));
    s.num_instances = num_instances; s.num_objects = num_objects; s.num_object_lights = d->num_lights;
    s.dev.lights = s.world_lights;
    s.dev.num_tris = d->num_tris; s.dev.num_materials = d->num_materials; s.dev.num_lights = (int32_t)world_lights;
    s.dev.top_image = s.dev.top_image_large = nullptr;         // the instanced kernels stage no image; no other kernel is launched
    HIP_CHECK(hipDeviceSynchronize());
    const int32_t rc = derive_instanced(dev, s, nullptr);
    int32_t info[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipDeviceSynchronize());
    if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(info, s.tlas_info, sizeof(info), hipMemcpyDeviceToHost));
    if (rc != RODENT_BUILD_OK || info[2]) return fail(rc != RODENT_BUILD_OK ? rc : info[2]);
    upload_shading_records(s, d, textured);
    s.inst.tlas = s.tlas_nodes; s.inst.instances = s.instances; s.inst.bases = s.bases;
    s.num_nodes = (int)total_nodes; s.num_bvh_tris = d->num_tris; s.num_vertices = d->num_vertices; s.tri_delta = 0;
    s.loaded = true; s.instanced = true;
    ensure_ray_slots(r, 0);
    r.mapping = resolve_mapping(r); r.trace_persistent = resolve_trace(r); resolve_refill(r);
    return RODENT_SCENE_OK;
}

extern "C" {

int32_t rodent_hip_scene_create_instanced(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                                          const RodentInstanceDesc* instances, int32_t num_instances, const RodentBuildOptions* opt) {
    return create_instanced_scene(dev, d, objects, num_objects, instances, num_instances, opt);
}

int32_t rodent_hip_scene_create_motion(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                                       const RodentMotionInstanceDesc* instances, int32_t num_instances, const RodentBuildOptions* opt) {
    return create_instanced_scene(dev, d, objects, num_objects, instances, num_instances, opt);
}

int32_t rodent_hip_scene_create_flags(int32_t dev) { return rdev(dev).create_flags; }

void rodent_hip_scene_set_motion_transforms(int32_t dev, const float* m0_dev, const float* m1_dev, void* stream_) {
    DevScene& s = motion_scene(dev, "rodent_hip_scene_set_motion_transforms");
    RenderDevice& r = rdev(dev);
    if (!m0_dev || !m1_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_set_motion_transforms: NULL matrices\n"); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    if (!r.ev_refit) HIP_CHECK(hipEventCreateWithFlags(&r.ev_refit, hipEventDisableTiming));
    hipStream_t stream = (hipStream_t)stream_;
    // behind the last move, whichever stream it took; frames need no wait (rodent_hip_scene_refit_device says why)
    if (s.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    hipLaunchKernelGGL(k_motion_instance_matrices, dim3((unsigned)((24 * s.num_instances + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                       m0_dev, m1_dev, s.num_instances, s.motion_descs);
    const int32_t rc = derive_instanced(dev, s, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: top-level rebuild refused (%d)\n", rc); abort(); }
    HIP_CHECK(hipEventRecord(r.ev_refit, stream));
    s.refit_enqueued = true;
}

void rodent_hip_scene_motion_instances(int32_t dev, RodentSceneMotionInstances* out) {
    DevScene& s = motion_scene(dev, "rodent_hip_scene_motion_instances");
    if (!out) return;
    ensure_ray_slots(rdev(dev), 0);
    *out = RodentSceneMotionInstances{s.tlas_nodes, s.motion_instances, s.motion_descs, s.objects, s.slot_of,
        reinterpret_cast<int32_t*>(s.bases), s.light_owner, s.world_lights, s.object_lights, s.inst.ray_slots, s.tlas_info, s.num_instances,
        s.num_objects, std::max(1, s.num_instances - 1), s.dev.num_lights, s.num_object_lights, (int32_t)s.ray_slot_cap};
}

int32_t rodent_hip_render_shutter(int32_t dev, float open, float close) {
    RenderDevice& r = rdev(dev);
    if (!(0.0f <= open && open <= close && close <= 1.0f)) return RODENT_SCENE_ERR_SHUTTER;      // (a NaN fails a comparison)
    r.shutter[0] = open + 0.0f; r.shutter[1] = close + 0.0f;                                     // (a -0 becomes +0)
    return RODENT_SCENE_OK;
}
void rodent_hip_render_shutter_in_effect(int32_t dev, float out[2]) { const RenderDevice& r = rdev(dev);
    out[0] = r.shutter[0]; out[1] = r.shutter[1]; }
int32_t rodent_hip_render_max_path_len_in_effect(int32_t dev) { return path_len_in_effect(rdev(dev)); }

void rodent_hip_scene_set_transforms(int32_t dev, const float* object_to_world_dev, void* stream_) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_set_transforms");
    RenderDevice& r = rdev(dev);
    if (!object_to_world_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_set_transforms: NULL matrices\n"); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    if (!r.ev_refit) HIP_CHECK(hipEventCreateWithFlags(&r.ev_refit, hipEventDisableTiming));
    hipStream_t stream = (hipStream_t)stream_;
    // behind the last move, whichever stream it took; frames need no wait (rodent_hip_scene_refit_device says why)
    if (s.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    hipLaunchKernelGGL(k_instance_matrices, dim3((unsigned)((12 * s.num_instances + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                       object_to_world_dev, s.num_instances, s.descs);
    const int32_t rc = derive_instanced(dev, s, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: top-level rebuild refused (%d)\n", rc); abort(); }
    HIP_CHECK(hipEventRecord(r.ev_refit, stream));
    s.refit_enqueued = true;
}

int32_t rodent_hip_scene_transforms_status(int32_t dev, int32_t* info) {
    DevScene& s = loaded_scene(dev, "rodent_hip_scene_transforms_status");
    if (!s.motion) instanced_scene(dev, "rodent_hip_scene_transforms_status");       // (it serves a moving scene's moves too)
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipSetDevice(dev));
    if (s.refit_enqueued) HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
    HIP_CHECK(hipMemcpy(words, s.tlas_info, sizeof(words), hipMemcpyDeviceToHost));
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    return words[2];
}

int32_t rodent_hip_scene_deform_prepare(int32_t dev, const int32_t* objects, int32_t num_objects, int32_t smooth_normals) {
    RenderDevice& r = rdev(dev);
    DevScene& s = r.scene;
    // ---- the refusals: on the host, the scene and an earlier set stay as they are ----
    if (!s.loaded || !s.instanced || s.motion) return RODENT_SCENE_ERR_NOT_INSTANCED;
    if (!objects || num_objects < 1) return RODENT_SCENE_ERR_COUNTS;
    std::vector<char> listed((size_t)s.num_objects, 0);
    for (int32_t k = 0; k < num_objects; k++) {
        if (objects[k] < 0 || objects[k] >= s.num_objects || listed[objects[k]]) return RODENT_SCENE_ERR_OBJECT;
        listed[objects[k]] = 1;
    }
    std::vector<int32_t> first_tri((size_t)num_objects), num_tris((size_t)num_objects);
    for (int32_t k = 0; k < num_objects; k++) {
        first_tri[k] = s.object_ranges[objects[k]].first_tri; num_tris[k] = s.object_ranges[objects[k]].num_tris; }
    std::vector<RodentRefitRange> ranges((size_t)num_objects);
    int32_t totals[2] = {};
    const int64_t scratch_bytes = rodent_hip_refit_objects_plan(s.object_table.data(), s.num_objects, objects, first_tri.data(),
                                                                num_tris.data(), num_objects, ranges.data(), totals);
    if (scratch_bytes < 0) return RODENT_SCENE_ERR_COUNTS;
    // ---- from here on the set is the new one ----
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());                   // no update still works in the lists that are replaced
    if (!r.ev_refit) HIP_CHECK(hipEventCreateWithFlags(&r.ev_refit, hipEventDisableTiming));
    for (void* p : s.deform.allocs) HIP_CHECK(hipFree(p));
    s.deform = DevScene::DeformSet();
    DevScene::DeformSet& d = s.deform;
    const auto put = [&](const auto* host, size_t count) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(host)>>;
        T* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(sizeof(T) * count, 16)));
        if (count) HIP_CHECK(hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice));
        d.allocs.push_back(p);
        return p;
    };
    d.ranges = put(ranges.data(), ranges.size());
    HIP_CHECK(hipMalloc(&d.scratch, (size_t)scratch_bytes + 4 * RODENT_BUILD_INFO_WORDS));
    d.allocs.push_back(d.scratch);
    d.info = reinterpret_cast<int32_t*>(d.scratch + scratch_bytes);
    HIP_CHECK(hipMemset(d.info, 0, 4 * RODENT_BUILD_INFO_WORDS));
    d.num_listed = num_objects; d.num_nodes = totals[0]; d.num_tris = totals[1]; d.smooth = smooth_normals != 0;
    // The tables the lists are made from never change under an update: indices, light ids, materials.
    const size_t nv = (size_t)s.num_vertices, nt = (size_t)s.dev.num_tris;
    std::vector<int32_t> indices(4 * nt), light_ids(nt);
    std::vector<RodentMaterial> materials((size_t)s.dev.num_materials);
    HIP_CHECK(hipMemcpy(indices.data(), s.dev.indices, sizeof(int32_t) * indices.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(light_ids.data(), s.dev.light_ids, sizeof(int32_t) * nt, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(materials.data(), s.dev.materials, sizeof(RodentMaterial) * materials.size(), hipMemcpyDeviceToHost));
    // light k of D's light ranges: bound to the lowest emissive triangle that names it (one of its own object's: the creation checked)
    std::vector<int2> bound;
    for (int32_t o = 0; o < s.num_objects; o++) {
        if (!listed[o]) continue;
        const RodentObjectRange& g = s.object_ranges[o];
        std::vector<int> tri((size_t)g.num_lights, -1);
        for (int32_t t = g.first_tri; t < g.first_tri + g.num_tris; t++) {
            const int32_t k = light_ids[t] - g.first_light;
            if (materials[indices[4 * (size_t)t + 3]].emissive && k >= 0 && k < g.num_lights && tri[k] < 0) tri[k] = t;
        }
        for (int32_t k = 0; k < g.num_lights; k++) if (tri[k] >= 0) bound.push_back(make_int2(g.first_light + k, tri[k]));
    }
    d.lights = put(bound.data(), bound.size()); d.num_lights = (int)bound.size();
    if (d.smooth) {
        // the vertices D's triangles name, ascending, and for each the corners of ALL triangles that name it, ascending (triangle, corner)
        std::vector<int> slot(nv, -1), verts;
        for (int32_t o = 0; o < s.num_objects; o++) {
            if (!listed[o]) continue;
            const RodentObjectRange& g = s.object_ranges[o];
            for (size_t c = 4 * (size_t)g.first_tri; c < 4 * (size_t)(g.first_tri + g.num_tris); c++) if (c % 4 != 3) slot[indices[c]] = 0;
        }
        for (size_t v = 0; v < nv; v++) if (slot[v] == 0) { slot[v] = (int)verts.size(); verts.push_back((int)v); }
        std::vector<int> first(verts.size() + 1, 0);
        for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) { const int j = slot[indices[4 * t + k]]; if (j >= 0) first[(size_t)j + 1]++; }
        for (size_t j = 0; j < verts.size(); j++) first[j + 1] += first[j];
        std::vector<int> next(first.begin(), first.end() - 1), tri((size_t)first.back());
        for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) { const int j = slot[indices[4 * t + k]]; if (j >= 0) tri[next[j]++] = (int)t; }
        d.verts = put(verts.data(), verts.size()); d.num_verts = (int)verts.size();
        d.corner_first = put(first.data(), first.size());
        d.corner_tri = put(tri.data(), tri.size());
    }
    return RODENT_SCENE_OK;
}

void rodent_hip_scene_deform_device(int32_t dev, const float* vertices_dev, const float* normals_dev, const float* object_to_world_dev,
                                    void* stream_) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_deform_device");
    RenderDevice& r = rdev(dev);
    DevScene::DeformSet& d = s.deform;
    if (!vertices_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_deform_device: NULL vertices\n"); abort(); }
    if (!d.ranges || (!normals_dev && !d.smooth)) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_deform_device: no deforming set declared (rodent_hip_scene_deform_prepare%s)\n",
                d.ranges ? " with smooth_normals, or pass normals" : ""); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)stream_;
    // behind the last update or move, whichever stream it took; frames need no wait (rodent_hip_scene_refit_device says why)
    if (s.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    const int nv = s.num_vertices;
    float4* const vertices = reinterpret_cast<float4*>(const_cast<float*>(s.dev.vertices));
    float4* const normals = reinterpret_cast<float4*>(const_cast<float*>(s.dev.normals));
    float4* const face_normals = reinterpret_cast<float4*>(const_cast<float*>(s.dev.face_normals));
    const int4* const indices = reinterpret_cast<const int4*>(s.dev.indices);
    if (vertices_dev != s.dev.vertices)
        HIP_CHECK(hipMemcpyAsync(vertices, vertices_dev, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToDevice, stream));
    if (normals_dev && normals_dev != s.dev.normals)
        HIP_CHECK(hipMemcpyAsync(normals, normals_dev, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToDevice, stream));
    const auto blocks = [](int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); };
    if (object_to_world_dev)
        hipLaunchKernelGGL(k_instance_matrices, blocks(12 * s.num_instances), dim3(kBlock), 0, stream, object_to_world_dev,
                           s.num_instances, s.descs);
    const DeformTris tris{d.ranges, d.num_listed, d.num_tris};
    hipLaunchKernelGGL(k_deform_face_normals, blocks(d.num_tris), dim3(kBlock), 0, stream, vertices, indices, tris, face_normals);
    if (d.num_lights > 0) hipLaunchKernelGGL(k_deform_light_records, blocks(d.num_lights), dim3(kBlock), 0, stream, vertices, indices,
                                             d.lights, d.num_lights, s.object_lights);
    if (!normals_dev) hipLaunchKernelGGL(k_deform_smooth_normals, blocks(d.num_verts), dim3(kBlock), 0, stream, face_normals, d.verts,
                                         d.corner_first, d.corner_tri, d.num_verts, normals);
    // the listed objects' hierarchies, in the packed allocation: rodent_hip_scene_bvh's pointers stay valid
    int32_t rc = rodent_hip_refit_objects(dev, s.dev.vertices, nv, s.dev.indices, s.dev.num_tris, const_cast<Node2*>(s.dev.nodes),
                                          const_cast<Tri1*>(s.dev.tris), s.objects, s.num_objects, d.ranges, d.num_listed, d.num_nodes,
                                          d.num_tris, d.scratch, d.info, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: refit of the deforming objects refused (%d)\n", rc); abort(); }
    if (s.dev.tri_shade) hipLaunchKernelGGL(k_deform_tri_shade, blocks(d.num_tris), dim3(kBlock), 0, stream, face_normals, normals,
                                            indices, tris, const_cast<float4*>(s.dev.tri_shade));
    // the objects' boxes changed: the TLAS, slot_of and the world lights, as after a move
    rc = derive_instanced(dev, s, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: top-level rebuild refused (%d)\n", rc); abort(); }
    HIP_CHECK(hipEventRecord(r.ev_refit, stream));
    s.refit_enqueued = true; d.enqueued = true;
}

int32_t rodent_hip_scene_deform_status(int32_t dev, int32_t* refit_info, int32_t* tlas_info) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_deform_status");
    const DevScene::DeformSet& d = s.deform;
    int32_t refit[RODENT_BUILD_INFO_WORDS] = {d.num_nodes, d.num_tris, 0, 0}, tlas[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipSetDevice(dev));
    if (s.refit_enqueued) HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
    if (d.enqueued) HIP_CHECK(hipMemcpy(refit, d.info, sizeof(refit), hipMemcpyDeviceToHost));    // before the first: a sound one's words
    HIP_CHECK(hipMemcpy(tlas, s.tlas_info, sizeof(tlas), hipMemcpyDeviceToHost));
    if (refit_info) std::copy(refit, refit + RODENT_BUILD_INFO_WORDS, refit_info);
    if (tlas_info) std::copy(tlas, tlas + RODENT_BUILD_INFO_WORDS, tlas_info);
    return refit[2] | tlas[2] | (refit[0] < d.num_nodes ? (int32_t)0x80000000u : 0);
}

void rodent_hip_scene_instances(int32_t dev, RodentSceneInstances* out) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_instances");
    if (!out) return;
    ensure_ray_slots(rdev(dev), 0);
    *out = RodentSceneInstances{s.tlas_nodes, s.instances, s.descs, s.objects, s.slot_of, reinterpret_cast<int32_t*>(s.bases),
        s.light_owner, s.world_lights, s.object_lights, s.inst.ray_slots, s.tlas_info, s.num_instances, s.num_objects,
        std::max(1, s.num_instances - 1), s.dev.num_lights, s.num_object_lights, (int32_t)s.ray_slot_cap};
}

void rodent_hip_render_config(int32_t dev, int32_t spp, int32_t max_path_len) {
    if (spp < 1 || max_path_len < 0) { fprintf(stderr, "rodent_hip: invalid render configuration\n"); abort(); }
    RenderDevice& r = rdev(dev); r.spp = spp; r.max_path_len = max_path_len;
}

void rodent_hip_render_sort(int32_t dev, int32_t enable) { rdev(dev).sort = enable ? 1 : 0; }
int32_t rodent_hip_render_sort_in_effect(int32_t dev) { return sort_in_effect(rdev(dev)); }
int32_t rodent_hip_render_trace_persistent_in_effect(int32_t dev) { return rdev(dev).trace_persistent; }
void rodent_hip_render_hit_records(int32_t dev, int32_t aos) { rdev(dev).hit_records_aos = aos ? 1 : 0; }
void rodent_hip_render_overlap(int32_t dev, int32_t enable) { rdev(dev).overlap = enable ? 1 : 0; }
void rodent_hip_render_fused_sort(int32_t dev, int32_t enable) { rdev(dev).fused_sort = enable ? 1 : 0; }
void rodent_hip_render_fused_compact(int32_t dev, int32_t enable) { rdev(dev).fused_compact = std::min(2, std::max(0, (int)enable)); }
void rodent_hip_render_lds_image(int32_t dev, int32_t enable) { rdev(dev).lds_image = enable ? 1 : 0; }
void rodent_hip_render_mega_joint(int32_t dev, int32_t enable) { rdev(dev).mega_joint = enable ? 1 : 0; }
void rodent_hip_render_trace_persistent(int32_t dev, int32_t enable) { RenderDevice& r = rdev(dev);
    r.trace_persistent_request = std::min(2, std::max(-1, (int)enable)); r.trace_persistent = resolve_trace(r); }

void rodent_hip_render_trace_refill(int32_t dev, int32_t idle_bounce, int32_t idle_shadow) {
    const bool per_scene = idle_bounce == -1 && idle_shadow == -1, off = idle_bounce == 0 && idle_shadow == 0;
    if (!per_scene && !off && (idle_bounce < 1 || idle_bounce > kWave || idle_shadow < 1 || idle_shadow > kWave)) {
        fprintf(stderr, "rodent_hip: lane refill thresholds must be -1, -1 (per scene), 0, 0 (off) or 1 .. 64 idle lanes each\n"); abort();
    }
    RenderDevice& r = rdev(dev);
    r.trace_refill_request[0] = idle_bounce; r.trace_refill_request[1] = idle_shadow;
    resolve_refill(r);
}

void rodent_hip_render_persist_min_rays(int32_t dev, int32_t rays) { rdev(dev).persist_min_rays = rays < 0 ? kPersistMinRays : rays; }
int32_t rodent_hip_render_persist_min_rays_in_effect(int32_t dev) { return rdev(dev).persist_min_rays; }
const char* rodent_hip_render_trace_kernel_name(int32_t dev) { return rdev(dev).trace_kernel; }

int32_t rodent_hip_render_trace_refill_in_effect(int32_t dev) { const RenderDevice& r = rdev(dev);
    return r.trace_refill | (r.trace_refill_shadow << 8); }

void rodent_hip_render_capacity(int32_t dev, int32_t rays) {
    if (rays != 0 && (rays < 64 || rays > kMaxCapacity)) {
        fprintf(stderr, "rodent_hip: stream capacity must be 0 (default) or 64 .. %ld rays\n", kMaxCapacity); abort(); }
    rdev(dev).capacity = rays;
}

void rodent_hip_render_mapping(int32_t dev, int32_t mapping) {
    if (mapping < -1 || mapping > 1) {
        fprintf(stderr, "rodent_hip: unknown mapping %d (-1 = per scene, 0 = streaming, 1 = megakernel)\n", mapping); abort(); }
    RenderDevice& r = rdev(dev);
    r.mapping_request = mapping;
    r.mapping = resolve_mapping(r);
}
int32_t rodent_hip_render_mapping_in_effect(int32_t dev) { return rdev(dev).mapping; }
void rodent_hip_render_defaults(int32_t dev) { RenderDevice& r = rdev(dev); render_defaults(r); r.mapping = resolve_mapping(r);
    r.trace_persistent = resolve_trace(r); resolve_refill(r); }

int32_t get_spp(void) { return rdev(g_current_dev).spp; }

void setup_interface(size_t width, size_t height) { g_host_w = width; g_host_h = height; g_host_film.assign(width * height * 3, 0.0f); }
float* get_pixels(void) { return g_host_film.data(); }
void cleanup_interface(void) {
    // buffers / BVHs / images loaded through rodent_load_* (services.hip)
    rodent_services_cleanup();
    for (auto& r : g_rdev) if (r.init && r.film) { (void)hipSetDevice(r.dev); (void)hipFree(r.film); r.film = nullptr;
        r.film_w = r.film_h = 0; }
    g_host_film.clear(); g_host_w = g_host_h = 0;
}
void clear_pixels(void) {                                                    // interface.cpp:498-505
    std::fill(g_host_film.begin(), g_host_film.end(), 0.0f);
    for (auto& r : g_rdev) if (r.init && r.film) { HIP_CHECK(hipSetDevice(r.dev));
        HIP_CHECK(hipMemset(r.film, 0, sizeof(float) * 3 * (size_t)r.film_w * r.film_h)); }
}

void rodent_get_film_data(int32_t dev, float** pixels, int32_t* width, int32_t* height) {
    RenderDevice& r = rdev(dev); ensure_film(r);
    *pixels = r.film; *width = r.film_w; *height = r.film_h;
}
void rodent_gpu_get_first_primary_stream(int32_t dev, PrimaryStream* p, int32_t size) { RenderDevice& r = rdev(dev);
    carve_primary(*p, ensure_slab(r, 0, size, 20), round_cap(size)); }
void rodent_gpu_get_second_primary_stream(int32_t dev, PrimaryStream* p, int32_t size) { RenderDevice& r = rdev(dev);
    carve_primary(*p, ensure_slab(r, 1, size, 20), round_cap(size)); }
void rodent_gpu_get_secondary_stream(int32_t dev, SecondaryStream* s, int32_t size) { RenderDevice& r = rdev(dev);
    carve_secondary(*s, ensure_slab(r, 2, size, 13), round_cap(size)); }
void rodent_gpu_get_tmp_buffer(int32_t dev, int32_t** buf, int32_t size) {
    RenderDevice& r = rdev(dev);
    *buf = r.growing(r.tmp, round_cap(size)).ensure(round_cap(size));
}
// Host stream slabs with the same carving (interface.cpp:367-373,621-629).  The library computes nothing on the CPU;
// a host that stages rays itself (or the reference's CPU mapping) gets the layout it expects.
void rodent_cpu_get_primary_stream(PrimaryStream* p, int32_t size) {
    const size_t cap = (size_t)round_cap(size);
    if (t_cpu_primary.size() < cap * 20) t_cpu_primary.assign(cap * 20, 0.0f);
    carve_primary(*p, t_cpu_primary.data(), t_cpu_primary.size() / 20);
}
void rodent_cpu_get_secondary_stream(SecondaryStream* s, int32_t size) {
    const size_t cap = (size_t)round_cap(size);
    if (t_cpu_secondary.size() < cap * 13) t_cpu_secondary.assign(cap * 13, 0.0f);
    carve_secondary(*s, t_cpu_secondary.data(), t_cpu_secondary.size() / 13);
}
void rodent_present(int32_t dev) {                                           // interface.cpp:494-496,660-663
    RenderDevice& r = rdev(dev);
    if (!r.film) return;
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipMemcpy(g_host_film.data(), r.film, sizeof(float) * 3 * (size_t)r.film_w * r.film_h, hipMemcpyDeviceToHost));
}

void rodent_hip_render_rows(int32_t dev, const Settings* settings, int32_t iter, int32_t y0, int32_t y1, void* stream) {
    RenderDevice& r = rdev(dev);
    ensure_film(r);
    if (y0 < 0 || y1 > r.film_h || y0 > y1) { fprintf(stderr, "rodent_hip: invalid row range [%d, %d)\n", y0, y1); abort(); }
    render_rows_any(r, settings, iter, y0, y1, (hipStream_t)stream);
}

// Interleaved row tiles (the reference hands out ~1024-sample tiles dynamically, render/mapping_gpu.impala:374-420,
// mapping_cpu.impala:200-237): this call renders the row tiles first_tile, first_tile + tile_stride, ... of tile_rows rows each -- GPU k of
// K takes first_tile = k, tile_stride = K. Seeds depend on absolute (sample, iter, x, y) only: the tiles of all GPUs together are the frame
// render() produces.
void rodent_hip_render_tiles(int32_t dev, const Settings* settings, int32_t iter, int32_t tile_rows, int32_t first_tile,
    int32_t tile_stride, void* stream) {
    RenderDevice& r = rdev(dev);
    ensure_film(r);
    if (tile_rows <= 0 || first_tile < 0 || tile_stride <= 0) {
        fprintf(stderr, "rodent_hip: invalid tile arguments (%d rows, first %d, stride %d)\n", tile_rows, first_tile, tile_stride);
        abort(); }
    const int full_tiles = r.film_h / tile_rows, ragged_rows = r.film_h % tile_rows;
    // complete tiles of this call
    const int mine = first_tile < full_tiles ? (full_tiles - first_tile + tile_stride - 1) / tile_stride : 0;
    const bool ragged_mine = ragged_rows > 0 && full_tiles >= first_tile && (full_tiles - first_tile) % tile_stride == 0;
    // the counters (rodent_hip_render_counters) are those of the whole call: its sub-calls after the first add to them
    r.counters_continue = false;
    // the megakernel tiles the rows it is given itself: one launch per row tile
    if (r.mapping == 1) {
        for (int k = 0; k < mine; k++) {
            render_rows_mega(r, settings, iter, (first_tile + k * tile_stride) * tile_rows, (first_tile + k * tile_stride + 1) * tile_rows,
            (hipStream_t)stream); r.counters_continue = true; }
    } else if (mine > 0) {
        const int y0 = first_tile * tile_rows;
        render_rows(r, settings, iter, y0, y0 + mine * tile_rows, (hipStream_t)stream, tile_rows, tile_stride * tile_rows);
        r.counters_continue = true;
    }
    if (ragged_mine) render_rows_any(r, settings, iter, full_tiles * tile_rows, r.film_h, (hipStream_t)stream);
    r.counters_continue = false;
}

void render(const Settings* settings, int32_t iter) {                        // generated render(): converter.cpp:628-967
    RenderDevice& r = rdev(g_current_dev);
    ensure_film(r);
    render_rows_any(r, settings, iter, 0, r.film_h, nullptr);
    rodent_present(g_current_dev);                                           // device.present() (converter.cpp:965)
}

void rodent_hip_render_counters(int32_t dev, uint64_t* out4) {
    RenderDevice& r = rdev(dev);
    HIP_CHECK(hipSetDevice(dev));
    uint64_t all[kNumCounters];
    HIP_CHECK(hipMemcpy(all, r.counters, sizeof(all), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out4[k] = all[k];
    for (int k = 4; k < 68; k++) out4[1] += all[k];                         // shadow rays are counted in 64 stripes
    for (int k = 68; k < kNumCounters; k++) out4[0] += all[k];              // the megakernel's primary rays, 32 stripes
}

// ---- stage-level entry points ---------------------------------------------------------------
void hip_generate_rays(int32_t dev, PrimaryStream* primary, int32_t capacity, int32_t first_ray_id, int32_t num_rays,
    const Settings* settings,
                       int32_t iter, int32_t film_width, int32_t film_height, int32_t first_pixel, int32_t spp, void* stream) {
    rdev(dev); HIP_CHECK(hipSetDevice(dev));
    if (primary->size + num_rays > capacity) { fprintf(stderr, "rodent_hip: hip_generate_rays exceeds the stream capacity\n"); abort(); }
    if (num_rays > 0)
        hipLaunchKernelGGL(generate_kernel(rdev(dev)), dim3((num_rays + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, *primary,
            primary->size, first_ray_id,
                           num_rays, to_cam(settings), iter, film_width, film_height, first_pixel, spp, 0, 0, 0, 0);
    primary->size += num_rays;
    HIP_CHECK(hipGetLastError());
}

void hip_traverse_primary(int32_t dev, PrimaryStream* primary, void* stream) {
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    if (primary->size <= 0) return;
    // a caller's stream holds its hit records in the ABI's five arrays (store_hit_record)
    primary->pad = 0;
    launch_trace(r, (hipStream_t)stream, {primary, primary->size, -1}, {});
    HIP_CHECK(hipGetLastError());
}

void hip_sort_primary(int32_t dev, PrimaryStream* primary, PrimaryStream* other, int32_t* ray_ends, void* stream) {
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    const int G = r.scene.dev.num_materials;
    if (G + 1 > kMaxBins) { fprintf(stderr, "rodent_hip: too many geometries (%d)\n", G); abort(); }
    bin_stream(r, 0, *primary, *other, nullptr, primary->size, KEY_GEOM, G + 1, 1, G + 1, (hipStream_t)stream);
    HIP_CHECK(hipMemcpyAsync(r.host_pinned + 8, bin_end(r, 0), sizeof(int) * (G + 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    std::memcpy(ray_ends, r.host_pinned + 8, sizeof(int) * (G + 1));
    other->size = primary->size;
}

void hip_shade(int32_t dev, PrimaryStream* primary, SecondaryStream* secondary, int32_t num_rays, void* stream) {
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    primary->size = num_rays; secondary->size = num_rays; primary->pad = 0;
    if (num_rays <= 0) return;
    if (r.scene.instanced) ensure_ray_slots(r, (size_t)num_rays);
    launch_shader(r, (hipStream_t)stream, shade_block(), num_rays, r.scene.dev, *primary, *primary, (const int*)nullptr, *secondary,
        (const int*)nullptr, num_rays, r.film,
                   1.0f / (float)r.spp, path_len_in_effect(r),
                       /* a ray that missed ends here instead of indexing the material table with the miss id: */ 1, (unsigned*)nullptr,
                       (int*)nullptr);
    HIP_CHECK(hipGetLastError());
}

int32_t hip_shade_compact(int32_t dev, PrimaryStream* from, PrimaryStream* to, SecondaryStream* secondary, const int32_t* perm,
    int32_t num_rays, int32_t mode, int32_t block, void* stream) {
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    if ((mode != 1 && mode != 2) || (block != 0 && block != 256 && block != 512 && block != 1024) || from->rays.id == to->rays.id) {
        fprintf(stderr, "rodent_hip: hip_shade_compact: mode must be 1 or 2, block 0, 256, 512 or 1024, and `to` another stream than "
        "`from` (mode %d, block %d)\n", mode, block); abort(); }
    from->size = num_rays; secondary->size = num_rays; from->pad = 0; to->pad = 0; to->size = 0;
    if (num_rays <= 0) return 0;
    const int b = block ? block : shade_block(), blocks = (num_rays + b - 1) / b;
    if (r.scene.instanced) ensure_ray_slots(r, (size_t)num_rays);
    int* d_alive = r.ctl + 6;                            // as in render_rows: the slot counter / the last block's new size
    HIP_CHECK(hipMemsetAsync(d_alive, 0, sizeof(int), (hipStream_t)stream));
    if (mode == 1) {
        r.growing(r.scan, blocks).ensure(blocks);
        HIP_CHECK(hipMemsetAsync(r.scan.ptr, 0, sizeof(unsigned) * (size_t)blocks, (hipStream_t)stream));
    }
    launch_shader(r, (hipStream_t)stream, b, num_rays, r.scene.dev, *from, *to, (const int*)perm, *secondary, (const int*)nullptr, num_rays,
        r.film, 1.0f / (float)r.spp, path_len_in_effect(r), 1, mode == 2 ? kScanAtomic : r.scan.ptr, d_alive);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(r.host_pinned + 8, d_alive, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    to->size = r.host_pinned[8];
    return to->size;
}

void hip_traverse_secondary(int32_t dev, SecondaryStream* secondary, void* stream) {
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    if (secondary->size <= 0) return;
    launch_trace(r, (hipStream_t)stream, {}, {secondary, nullptr, secondary->size, 1.0f / (float)r.spp});
    HIP_CHECK(hipGetLastError());
}

int32_t hip_traverse_streams(int32_t dev, PrimaryStream* primary, int32_t coherent_from, SecondaryStream* secondary,
    const int32_t* shadow_size_dev, int32_t flags, void* stream) {
    if (!primary && !secondary) return -1;
    if ((flags & ~kHitRecordsAoS) || (primary && primary->size < 0) || (secondary && secondary->size < 0)) return -2;
    if (primary && coherent_from > primary->size) return -3;
    StreamSlab slab;
    if ((flags & kHitRecordsAoS) && (!primary || !stream_slab(*primary, slab) || !slab.base)) return -4;
    RenderDevice& r = open_scene(rdev(dev), (hipStream_t)stream);
    // an empty list is no pass (the one-chunk kernels have no launch of zero workgroups)
    PrimaryStream p{};
    if (primary && primary->size > 0) { p = *primary; p.pad = flags & kHitRecordsAoS; }
    const ClosestPass c = p.size > 0 ? ClosestPass{&p, p.size, coherent_from} : ClosestPass{};
    const ShadowPass sh = secondary && secondary->size > 0 ? ShadowPass{secondary, shadow_size_dev, secondary->size, 1.0f / (float)r.spp}
        : ShadowPass{};
    if (!c.p && !sh.s) return 0;
    launch_trace(r, (hipStream_t)stream, c, sh);
    HIP_CHECK(hipGetLastError());
    return 0;
}

int32_t hip_compact_primary(int32_t dev, PrimaryStream* primary, PrimaryStream* other, void* stream) {
    RenderDevice& r = rdev(dev); HIP_CHECK(hipSetDevice(dev));
    bin_stream(r, 1, *primary, *other, nullptr, primary->size, KEY_ALIVE, 2, 0, 1, (hipStream_t)stream);
    HIP_CHECK(hipMemcpyAsync(r.host_pinned + 8, bin_end(r, 1), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    other->size = r.host_pinned[8];
    return other->size;
}

int32_t hip_bin_primary(int32_t dev, PrimaryStream* from, PrimaryStream* to, int32_t mode, int32_t num_bins, int32_t drop_from_bin,
    int32_t keep_hit, int32_t copy_interval, int32_t* perm, const int32_t* size_dev, int32_t max_n, int32_t* bin_ends, void* stream) {
    RenderDevice& r = rdev(dev); HIP_CHECK(hipSetDevice(dev));
    if ((mode != KEY_GEOM && mode != KEY_ALIVE) || num_bins < 1 || num_bins > kMaxBins || drop_from_bin < 1 || drop_from_bin > num_bins ||
        max_n < 0 || (!perm && from->rays.id == to->rays.id) || ((from->pad | to->pad) & kHitRecordsAoS)) {
        fprintf(stderr, "rodent_hip: hip_bin_primary: mode must be 0 or 1, num_bins 1 ... %d, drop_from_bin 1 ... num_bins, max_n >= 0, "
        "`to` another stream than `from` unless `perm` is given, and both streams with their hit records in the five arrays (mode %d, "
        "num_bins %d, drop_from_bin %d, max_n %d)\n", kMaxBins, mode, num_bins, drop_from_bin, max_n); abort(); }
    // the bin arrays the renderer's loop uses for that key: set 0 = sort by geometry, set 1 = compaction
    bin_stream(r, mode, *from, *to, size_dev, max_n, mode, num_bins, keep_hit, drop_from_bin, (hipStream_t)stream, copy_interval, perm);
    HIP_CHECK(hipMemcpyAsync(r.host_pinned + 8, bin_end(r, mode), sizeof(int) * num_bins, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    std::memcpy(bin_ends, r.host_pinned + 8, sizeof(int) * num_bins);
    return r.host_pinned[8 + drop_from_bin - 1];
}

} // extern "C"
