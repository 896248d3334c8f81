// render_sort.h -- the renderer's binning stage (K4 / K7): the deterministic sort by geometry id and the compaction, k_bin_count /
// k_bin_scan_blocks / k_bin_scan_bins / k_scatter.
//
// Included by render.hip inside its anonymous namespace (after the constants and stream_size).
#pragma once

// ---------------------------------------------------------------------------------------------
// K4 / K7: deterministic, stable binning of a primary stream (sort by geometry id, or compaction
// with key = dead ? 1 : 0).  dst(ray) = bin_begin[key] + (rays with that key in earlier blocks)
//                                      + (rank among the block's rays with that key).
// The reference uses one global atomic per ray for both (mapping_gpu.impala:195,217,293), which
// serialises and makes the output order nondeterministic.
// ---------------------------------------------------------------------------------------------
enum KeyMode { KEY_GEOM = 0, KEY_ALIVE = 1 };
__device__ __forceinline__ int stream_key(const PrimaryStream& p, int i, int mode) {
    return mode == KEY_GEOM ? p.geom_id[i] : (p.rays.id[i] >= 0 ? 0 : 1);
}

// in-block rank of thread `tid` among threads with the same key; also leaves the block's per-key counts in cnt[]
__device__ __forceinline__ int block_rank(int key, bool valid, int num_bins, int* cnt /* LDS [kBinBlock / kWave][num_bins] */) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int k = threadIdx.x; k < (kBinBlock / kWave) * num_bins; k += kBinBlock) cnt[k] = 0;
    __syncthreads();
    int rank = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                           // one round per distinct key present in the wave
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, leader);
        const unsigned long long same = __ballot(valid && key == k0);
        if (valid && key == k0) rank = __popcll(same & ((1ull << lane) - 1ull));
        if (lane == leader) cnt[wave * num_bins + k0] = __popcll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (valid) for (int w = 0; w < wave; w++) rank += cnt[w * num_bins + key];
    return rank;
}

// counts only (no ranks): 256 threads take the kBinBlock rays of one binning block four at a time; one LDS add per wave and
// distinct key.  (As a 1024-thread workgroup with the ranking of k_scatter it waited for sixteen free wave slots on one CU
// while the shadow-ray pass filled the chip on the other stream: 13 -> 98 ms per five cfg4 frames.)
__global__ __launch_bounds__(kBlock) void k_bin_count(PrimaryStream p, const int* size_ptr, int n_value, int mode, int num_bins,
    int num_blocks, int* hist /* [num_bins][num_blocks] */) {
    extern __shared__ int cnt[];
    const int n = stream_size(size_ptr, n_value);
    for (int k = threadIdx.x; k < num_bins; k += kBlock) cnt[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x % kWave;
    for (int r = 0; r < kBinBlock / kBlock; r++) {
        const int i = blockIdx.x * kBinBlock + r * kBlock + threadIdx.x;
        const bool valid = i < n;
        const int key = valid ? stream_key(p, i, mode) : 0;
        unsigned long long todo = __ballot(valid);
        while (todo) {                                       // one round per distinct key present in the wave
            const int leader = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(key, leader);
            const unsigned long long same = __ballot(valid && key == k0);
            if (lane == leader) atomicAdd(&cnt[k0], __popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < num_bins; k += kBlock) hist[(size_t)k * num_blocks + blockIdx.x] = cnt[k];
}

// one workgroup per bin: exclusive scan of that bin's per-block counts (in place), total -> bin_total[bin].
// Tiles of kBlock x kScanItems consecutive counts (16 per thread as four 16-byte loads), in-wave scan of the thread sums
// by lane shifts, waves joined through LDS, a running carry across tiles: 8 Mi rays = 32 768 counts per bin = 8 tiles.
// (The first version gave each thread one contiguous run of counts and scanned the 256 run sums serially on thread 0,
// the second scanned 256 counts per tile: with one workgroup per bin -- ten on the Cornell box -- both were a chain of
// 128+ dependent steps, 11 % of the frame.)
constexpr int kScanItems = 16;
__global__ __launch_bounds__(kBlock) void k_bin_scan_blocks(int* hist, int num_blocks, int* bin_total) {
    __shared__ int wave_sum[kBlock / kWave];
    int* row = hist + (size_t)blockIdx.x * num_blocks;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const bool aligned = (((size_t)row) & 15) == 0;
    int carry = 0;
    for (int tile = 0; tile < num_blocks; tile += kBlock * kScanItems) {
        const int b0 = tile + (int)threadIdx.x * kScanItems;
        int v[kScanItems];
        if (aligned && b0 + kScanItems <= num_blocks) {
#pragma unroll
            for (int k = 0; k < kScanItems / 4; k++) { const int4 x = *reinterpret_cast<const int4*>(row + b0 + 4 * k); v[4 * k] = x.x;
                v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w; }
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; k++) v[k] = b0 + k < num_blocks ? row[b0 + k] : 0;
        }
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) { const int x = v[k]; v[k] = sum; sum += x; }         // exclusive within the thread
        int incl = sum;
        for (int o = 1; o < kWave; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
        if (lane == kWave - 1) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kBlock / kWave; w++) { const int ws = wave_sum[w]; if (w < wave) before += ws; total += ws; }
        const int base = carry + before + incl - sum;
        if (aligned && b0 + kScanItems <= num_blocks) {
#pragma unroll
            for (int k = 0; k < kScanItems / 4; k++) *reinterpret_cast<int4*>(row + b0 + 4 * k) = make_int4(base + v[4 * k],
                base + v[4 * k + 1], base + v[4 * k + 2], base + v[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; k++) if (b0 + k < num_blocks) row[b0 + k] = base + v[k];
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) bin_total[blockIdx.x] = carry;
}

// single workgroup: exclusive scan over bins; bin_begin[k], bin_end[k] (= ray_ends of mapping_gpu.impala:203-207)
__global__ void k_bin_scan_bins(const int* bin_total, int num_bins, int* bin_begin, int* bin_end) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { int acc = 0; for (int k = 0; k < num_bins; k++) { bin_begin[k] = acc; acc += bin_total[k];
        bin_end[k] = acc; } }
}

// copy_primary_ray (mapping_gpu.impala:136-164) to the computed slot
__global__ __launch_bounds__(kBinBlock) void k_scatter(PrimaryStream p, PrimaryStream q, const int* size_ptr, int n_value, int mode,
    int num_bins, int num_blocks,
                                                     const int* hist, const int* bin_begin, int keep_hit, int drop_from_bin,
                                                         int copy_interval, int* __restrict__ perm) {
    extern __shared__ int cnt[];
    const int n = stream_size(size_ptr, n_value);
    const int i = blockIdx.x * kBinBlock + threadIdx.x;
    const bool valid = i < n;
    const int key = valid ? stream_key(p, i, mode) : 0;
    // ALL loads first -- and before the in-block ranking, whose two barriers and LDS rounds then overlap their latency -- then
    // all stores.  Written as q.x[d] = p.x[i] pairs the copy compiled to load - wait - store, one word at a time (p and q may
    // alias as far as the compiler knows, so no load moves above the store before it; 14 VGPRs): every word paid a full memory
    // latency and the kernel ran at 1.7 TB/s.
    const bool copy = valid && key < drop_from_bin && !perm;
    int id = 0; float ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0, tmin = 0, tmax = 0, t = 0, u = 0, v = 0, mis = 0, cr = 0, cg = 0,
        cb = 0;
    int geom = 0, prim = 0, depth = 0; uint32_t rnd = 0;
    int begin = 0, before = 0;
    if (valid && key < drop_from_bin) { begin = bin_begin[key]; before = hist[(size_t)key * num_blocks + blockIdx.x]; }
    if (copy) {
        id = p.rays.id[i];
        ox = p.rays.org_x[i]; oy = p.rays.org_y[i]; oz = p.rays.org_z[i]; dx = p.rays.dir_x[i]; dy = p.rays.dir_y[i]; dz = p.rays.dir_z[i];
        // the ray interval is dead between the traversal and the shader (which writes a new one for every ray that goes on):
        // the sort before shading (copy_interval == 0) leaves the two words behind -- 10 % of its traffic
        if (copy_interval) { tmin = p.rays.tmin[i]; tmax = p.rays.tmax[i]; }
        if (keep_hit) { geom = p.geom_id[i]; prim = p.prim_id[i]; t = p.t[i]; u = p.u[i]; v = p.v[i]; }
        rnd = p.rnd[i]; mis = p.mis[i]; cr = p.contrib_r[i]; cg = p.contrib_g[i]; cb = p.contrib_b[i]; depth = p.depth[i];
    }
    const int rank = block_rank(key, valid, num_bins, cnt);
    if (!valid || key >= drop_from_bin) return;
    const int d = begin + before + rank;
    if (perm) { perm[d] = i; return; }                          // index-only sort: the consumer gathers (k_shade)
    // (keeps the stores below the loads whatever the optimiser thinks of the pairs)
    asm volatile("" ::: "memory");
    q.rays.id[d] = id;
    q.rays.org_x[d] = ox; q.rays.org_y[d] = oy; q.rays.org_z[d] = oz; q.rays.dir_x[d] = dx; q.rays.dir_y[d] = dy; q.rays.dir_z[d] = dz;
    if (copy_interval) { q.rays.tmin[d] = tmin; q.rays.tmax[d] = tmax; }
    if (keep_hit) { q.geom_id[d] = geom; q.prim_id[d] = prim; q.t[d] = t; q.u[d] = u; q.v[d] = v; }
    q.rnd[d] = rnd; q.mis[d] = mis; q.contrib_r[d] = cr; q.contrib_g[d] = cg; q.contrib_b[d] = cb; q.depth[d] = depth;
}
