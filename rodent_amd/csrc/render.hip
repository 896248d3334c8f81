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
#include "traversal_motion_steps.h"

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
#include "render_deforming.h"

// ---------------------------------------------------------------------------------------------
// Host side: per-device state (interface.cpp:324-339), stream slabs, the streaming loop
// ---------------------------------------------------------------------------------------------
// The scene of a device: RenderDevice holds it by value, so it is declared here; all the code that works on it is render_scene.h's.
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
    // A DEFORMING scene (rodent_hip_scene_create_deforming) is a flat one that owns two keys: dev.vertices / dev.normals are the mesh at
    // time 0, `vertices1` / `normals1` the mesh at time 1, dev.nodes / dev.tris the static key-0 hierarchy -- the read-only topology of
    // every rebuild, which no kernel walks -- and `motion_nodes` / `motion_tris` the two-key records the frame traces, rebuilt by every
    // rodent_hip_scene_set_motion_keys with `motion_scratch` into `motion_info`.  `face_normals1`: key 1's face normals, scratch of the
    // smooth normals (key 0's go to dev.face_normals).  Neither `instanced` nor `motion` is set; everything is in `allocs`.
    bool deforming = false;
    RodentMotionNode2* motion_nodes = nullptr; RodentMotionTri1* motion_tris = nullptr;
    float *vertices1 = nullptr, *normals1 = nullptr, *face_normals1 = nullptr;
    char* motion_scratch = nullptr; int32_t* motion_info = nullptr;
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
// (nor is a deforming scene's time word, for which the sort is not built)
int sort_in_effect(const RenderDevice& r) { return r.scene.instanced || r.scene.deforming ? 0 : r.sort; }
// a scene whose paths carry a time: moving instances, or a deforming mesh
bool timed_scene(const RenderDevice& r) { return r.scene.motion || r.scene.deforming; }
// ... and about the path length: such a scene's depth word keeps eight bits for the depth
int path_len_in_effect(const RenderDevice& r) {
    return timed_scene(r) ? std::min(r.max_path_len, RODENT_MOTION_DEPTH_MASK) : r.max_path_len;
}
// the ray generation of the scene that is loaded
decltype(&k_generate<false>) generate_kernel(const RenderDevice& r) { return timed_scene(r) ? k_generate<true> : k_generate<false>; }
// what the kernels of a moving scene take beside SceneDev: the scene's tables and the shutter as it is now
MotionDev motion_dev(const RenderDevice& r) {
    const DevScene& s = r.scene;
    return MotionDev{s.tlas_nodes, s.motion_instances, s.bases, s.inst.ray_slots, r.shutter[0], r.shutter[1]};
}

// ... of a deforming scene: the motion records, key 1's tables and the shutter as it is now
DeformingDev deforming_dev(const RenderDevice& r) {
    const DevScene& s = r.scene;
    return DeformingDev{s.motion_nodes, s.motion_tris, s.vertices1, s.normals1, r.shutter[0], r.shutter[1]};
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
// (a deforming scene: the flat shader's form with ONE trailing DeformingDev argument)
template <typename... Args> void launch_k_shade_deforming(hipStream_t stream, int b, int rays, const DeformingDev& in, Args... args) {
    const int blocks = (rays + b - 1) / b;
    if (b == 256) hipLaunchKernelGGL((k_shade<256, false, DeformingDev>), dim3(blocks), dim3(256), 0, stream, args..., in);
    else if (b == 512) hipLaunchKernelGGL((k_shade<512, false, DeformingDev>), dim3(blocks), dim3(512), 0, stream, args..., in);
    else hipLaunchKernelGGL((k_shade<1024, false, DeformingDev>), dim3(blocks), dim3(1024), 0, stream, args..., in);
}
// the shader of the scene that is loaded
template <typename... Args> void launch_shader(RenderDevice& r, hipStream_t stream, int b, int rays, Args... args) {
    if (r.scene.deforming) launch_k_shade_deforming(stream, b, rays, deforming_dev(r), args...);
    else if (r.scene.motion) launch_k_shade_instanced(stream, b, rays, motion_dev(r), args...);
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
// A deforming scene: one launch per pass over the motion records, no follow-up kernel (render_deforming.h).
void launch_trace_deforming(RenderDevice& r, hipStream_t stream, const ClosestPass& c, const ShadowPass& sh) {
    const DevScene& s = r.scene;
    if (c.p) {
        r.trace_kernel = "k_trace_deforming<false>";
        hipLaunchKernelGGL(k_trace_deforming<false>, dim3((c.n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev, deforming_dev(r),
            *c.p, SecondaryStream{}, (const int*)nullptr, c.n, (float*)nullptr, 0.0f, r.counters, r.ctl + 2, r.ctl + 6);
    }
    if (sh.s) {
        r.trace_kernel = "k_trace_deforming<true>";
        hipLaunchKernelGGL(k_trace_deforming<true>, dim3((sh.max_n + kWave - 1) / kWave), dim3(kWave), 0, stream, s.dev,
            deforming_dev(r), PrimaryStream{}, *sh.s, sh.size_ptr, sh.max_n, r.film, sh.inv_spp, r.counters, r.ctl + 2, (int*)nullptr);
    }
}
void launch_trace(RenderDevice& r, hipStream_t stream, const ClosestPass& c, const ShadowPass& sh) {
    if (r.scene.deforming) { launch_trace_deforming(r, stream, c, sh); return; }
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
    if (r.scene.instanced || r.scene.deforming) return 0;      // the instanced and the deforming kernels are stream kernels
    if (r.mapping_request >= 0) return r.mapping_request;
    return r.scene.loaded && r.scene.num_nodes <= auto_mega_max_nodes() ? 1 : 0;
}
// The stream traversal launches of the streaming loop when the caller leaves the choice to the library: the joint persistent launch
// for every hierarchy above the megakernel's size class (+3 ... +9 % on the atrium at 306 ... 142 444 nodes, profiles/r03_joint_sweep.txt),
// the 2-wave kernels with the shadow pass on a second stream for a tree of a few dozen nodes (Cornell box: joint -5 %).
int resolve_trace(const RenderDevice& r) {
    if (r.scene.instanced || r.scene.deforming) return 0;
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
    if (r.scene.instanced || r.scene.deforming) { r.trace_refill = r.trace_refill_shadow = 0; return; }
    if (r.trace_refill_request[0] >= 0) { r.trace_refill = r.trace_refill_request[0]; r.trace_refill_shadow = r.trace_refill_request[1];
        return; }
    r.trace_refill = r.trace_refill_shadow = r.scene.loaded && r.scene.num_nodes >= kRefillMinNodes ? kRefillIdleLanes : 0;
}

// host-side stream slabs of rodent_cpu_get_*_stream: per thread, like the reference's (interface.cpp:341-342,507-508)
thread_local std::vector<float> t_cpu_primary, t_cpu_secondary;

} // namespace

void rodent_services_cleanup();                                              // services.hip

// The scene: everything that creates, checks, updates, reports on or destroys a DevScene, and its entry points.
#include "render_scene.h"

extern "C" {

void rodent_hip_set_device(int32_t dev) { rdev(dev); g_current_dev = dev; }

int32_t rodent_hip_render_shutter(int32_t dev, float open, float close) {
    RenderDevice& r = rdev(dev);
    if (!(0.0f <= open && open <= close && close <= 1.0f)) return RODENT_SCENE_ERR_SHUTTER;      // (a NaN fails a comparison)
    r.shutter[0] = open + 0.0f; r.shutter[1] = close + 0.0f;                                     // (a -0 becomes +0)
    return RODENT_SCENE_OK;
}
void rodent_hip_render_shutter_in_effect(int32_t dev, float out[2]) { const RenderDevice& r = rdev(dev);
    out[0] = r.shutter[0]; out[1] = r.shutter[1]; }
int32_t rodent_hip_render_max_path_len_in_effect(int32_t dev) { return path_len_in_effect(rdev(dev)); }

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
void rodent_hip_render_defaults(int32_t dev) { RenderDevice& r = rdev(dev); render_defaults(r); resolve_options(r); }

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
