// build_ploc.h -- the PLOC topology stage of the device BVH builder (included by bvh_build.hip after build_split.h).
#pragma once
// ---- 10. topology by parallel locally-ordered clustering (Meister & Bittner 2018) -----------------------------------------------------
// The rule is include/rodent_build.h's; tests/ploc_model.py restates it.  This stage stands where k_karras + k_explicit stand: from the
// sorted references' boxes it writes the explicit tree (left / right / parent / leaf_parent; ids 0 .. m-1 inner, m + p the sorted
// reference p) that the optimising tail fits, restructures, collapses and emits.
// Clusters (box, id, height: one 32-byte record) lie in Morton order in two buffers used in turn; in LDS a box is six planes (SoA), so
// lanes scanning neighbouring positions read neighbouring banks.  state[2 * b], state[2 * b + 1]: the cluster count C and the iterations run t
// before device-wide iteration k, b = k & 1; every kernel of iteration k reads slot b, its compaction writes slot b ^ 1.  state[4 .. 6]:
// the buffer, C and t that k_ploc_shrink hands to k_ploc_finish.
// A device-wide iteration: k_ploc_nn, k_ploc_flags, k_scan, k_ploc_compact.  They are launched a host-known number of times on grids sized
// for the most references there can be and do nothing once C <= 1; k_ploc_shrink and k_ploc_finish, one workgroup each, then run the
// same rule to the end.
constexpr int kPlocMaxRadius = 64;
constexpr int kPlocFinish = 1024;                        // lanes of the finisher, and the most clusters it keeps in LDS
enum { kInfoIterations = 7 };

struct __attribute__((aligned(16))) PlocCluster { float box[6]; int id, h; };

struct Ploc {
    int n, m, radius, depth_limit, nblocks;              // nblocks = blocks of kBlock over the most references there can be
    const int* nref;                                     // the split front: n' references, on the device
    const float* leafbox;
    int *left, *right, *parent, *leaf_parent;
    PlocCluster *buf0, *buf1;                            // clusters by position, the two buffers
    int* nn;                                             // per position: the position it chose, -1 for none
    uint32_t* blocktot;                                  // nblocks leader counts, then nblocks survivor counts, scanned as one array
    int *state, *info;
};

__device__ __forceinline__ bool resolve(Ploc& p) {
    if (p.nref) { p.n = *p.nref; p.m = p.n - 1; }
    return p.m > 0;
}
__device__ __forceinline__ PlocCluster* ploc_buffer(const Ploc& p, int k) { return k ? p.buf1 : p.buf0; }
__device__ __forceinline__ int clog2(int x) { return x <= 1 ? 0 : 32 - __clz(x - 1); }
__device__ __forceinline__ int ploc_nn_iterations(int n) { return 4 * clog2(n) + 8; }

// The choice of position i among C clusters: the admissible position within `radius` whose union with i has the least half area, equal
// areas to the smaller i ^ j, never a NaN; -1 when there is none.  hcap = D - clog2(C).  Bound k of position j's box is
// bx[k * ks + (j - base) * js] and its height hh[(j - base) * js]: planes in LDS (js = 1) or the records in global memory (ks = 1, js = 8).
__device__ __forceinline__ int ploc_choose(int i, int C, int radius, int hcap, const float* bx, int ks, int js, const int* hh, int base) {
    float bi[6];
    for (int k = 0; k < 6; k++) bi[k] = bx[k * ks + (size_t)(i - base) * js];
    const int hi = hh[(size_t)(i - base) * js], from = max(i - radius, 0), to = min(i + radius, C - 1);
    int bj = -1;
    float bd = 0.0f;
    for (int j = from; j <= to; j++) {                   // selects only: the lanes of a wave stay together
        float u[6];
        for (int a = 0; a < 3; a++) {
            u[2 * a] = fminf(bi[2 * a], bx[(2 * a) * ks + (size_t)(j - base) * js]);
            u[2 * a + 1] = fmaxf(bi[2 * a + 1], bx[(2 * a + 1) * ks + (size_t)(j - base) * js]);
        }
        const float d = half_area(u);
        const bool ok = j != i && 1 + max(hi, hh[(size_t)(j - base) * js]) <= hcap && d == d;
        const bool better = ok && (bj < 0 || d < bd || (d == bd && (i ^ j) < (i ^ bj)));
        bd = better ? d : bd; bj = better ? j : bj;
    }
    return bj;
}
__device__ __forceinline__ int ploc_choose(int i, int C, int radius, int hcap, const PlocCluster* in) {
    return ploc_choose(i, C, radius, hcap, in[0].box, 1, 8, &in[0].h, 0);
}
// ... in a forced iteration: positions 2k and 2k + 1, a last odd one stays.
__device__ __forceinline__ int ploc_forced(int i, int C) { return (i ^ 1) < C ? (i ^ 1) : -1; }

// Leader (bit 16) and survivor (bit 0) of position i < C from the choices: i and j merge when each chose the other, the lower position
// leads and survives, the partner's slot is dropped.  *partner: j for a leader.
__device__ __forceinline__ uint32_t ploc_role(int i, const int* nn, int* partner) {
    const int j = nn[i];
    const bool merged = j >= 0 && nn[j] == i;
    *partner = j;
    return merged ? (i < j ? 0x10001u : 0u) : 1u;
}

// The cluster a survivor becomes: with `lead`, the merge of a (the leader) and b as inner node `node`, whose links are written;
// otherwise a itself (b is then a too: a box united with itself stays as it is, so both take one path).
__device__ __forceinline__ PlocCluster ploc_survivor(const Ploc& p, bool lead, int node, const PlocCluster& a, const PlocCluster& b) {
    PlocCluster c;
    unite(c.box, a.box, b.box);
    c.id = lead ? node : a.id; c.h = lead ? 1 + max(a.h, b.h) : a.h;
    if (lead) {
        p.left[node] = a.id; p.right[node] = b.id;
        if (a.id < p.m) p.parent[a.id] = node; else p.leaf_parent[a.id - p.m] = node;
        if (b.id < p.m) p.parent[b.id] = node; else p.leaf_parent[b.id - p.m] = node;
    }
    return c;
}

// The clusters of iteration 0: every sorted reference, its box, height 0.
__global__ __launch_bounds__(kBlock) void k_ploc_init(Ploc p) {
    const bool tree = resolve(p);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        p.state[0] = p.n; p.state[1] = 0;
        if (!p.nref) p.info[kInfoRefs] = p.n;
        if (tree) p.parent[0] = -1;
    }
    if (!tree || i >= p.n) return;
    PlocCluster c;
    for (int k = 0; k < 6; k++) c.box[k] = p.leafbox[6 * (size_t)i + k];
    c.id = p.m + i; c.h = 0;
    p.buf0[i] = c;
}

// Neighbour search of device-wide iteration k: a block stages its 256 positions and a halo of `radius` on each side in LDS.
__global__ __launch_bounds__(kBlock) void k_ploc_nn(Ploc p, int k) {
    constexpr int kSpan = kBlock + 2 * kPlocMaxRadius;
    __shared__ float sb[6 * kSpan];
    __shared__ int sh[kSpan];
    if (!resolve(p)) return;
    const int cur = k & 1, C = p.state[2 * cur], t = p.state[2 * cur + 1], block0 = blockIdx.x * kBlock;
    if (C <= 1 || block0 >= C) return;                   // uniform over the block
    const int i = block0 + threadIdx.x;
    if (t >= ploc_nn_iterations(p.n)) {
        if (i < C) p.nn[i] = ploc_forced(i, C);
        return;
    }
    const PlocCluster* in = ploc_buffer(p, cur);
    const int base = block0 - p.radius, span = kBlock + 2 * p.radius;
    for (int s = threadIdx.x; s < span; s += kBlock) {
        const int j = base + s;
        if (j < 0 || j >= C) continue;
        const PlocCluster c = in[j];
        for (int a = 0; a < 6; a++) sb[a * kSpan + s] = c.box[a];
        sh[s] = c.h;
    }
    __syncthreads();
    if (i < C) p.nn[i] = ploc_choose(i, C, p.radius, (p.depth_limit ? p.depth_limit : kMaxDepth) - clog2(C), sb, kSpan, 1, sh, base);
}

// Leaders and survivors per block of 256 positions; a block past C (or every block, once C <= 1) counts none.
__global__ __launch_bounds__(kBlock) void k_ploc_flags(Ploc p, int k) {
    const bool tree = resolve(p);
    const int cur = k & 1, C = tree ? p.state[2 * cur] : 1, i = blockIdx.x * kBlock + threadIdx.x;
    int j;
    uint32_t total;
    block_scan(C > 1 && i < C ? ploc_role(i, p.nn, &j) : 0u, &total);
    if (threadIdx.x == 0) { p.blocktot[blockIdx.x] = total >> 16; p.blocktot[p.nblocks + blockIdx.x] = total & 0xFFFFu; }
}

// The compaction: merges write their links and the merged cluster, the other survivors move up; the next C and t.
__global__ __launch_bounds__(kBlock) void k_ploc_compact(Ploc p, int k) {
    const bool tree = resolve(p);
    const int cur = k & 1, nxt = cur ^ 1, C = tree ? p.state[2 * cur] : 1, t = tree ? p.state[2 * cur + 1] : 0;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (C <= 1) {
        if (i == 0) { p.state[2 * nxt] = C; p.state[2 * nxt + 1] = t; }
        return;
    }
    if ((int)(blockIdx.x * kBlock) >= C) return;         // uniform over the block
    if (i == 0) { p.state[2 * nxt] = C - (int)p.blocktot[p.nblocks]; p.state[2 * nxt + 1] = t + 1; }
    int j = -1;
    const uint32_t role = i < C ? ploc_role(i, p.nn, &j) : 0u;
    uint32_t total;
    const uint32_t before = block_scan(role, &total);
    if (!(role & 1u)) return;
    const bool lead = (role >> 16) != 0u;
    const int leaders = (int)(p.blocktot[blockIdx.x] + (before >> 16));
    const int q = (int)(p.blocktot[p.nblocks + blockIdx.x] - p.blocktot[p.nblocks] + (before & 0xFFFFu));
    const PlocCluster* in = ploc_buffer(p, cur);
    ploc_buffer(p, nxt)[q] = ploc_survivor(p, lead, (C - 2) - leaders, in[i], in[lead ? j : i]);
}

// Exclusive scan of v over the finisher's 1024 lanes, the total in *total; may be called again and again.
__device__ uint32_t ploc_scan(uint32_t v, uint32_t* total, uint32_t* wsum) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();                                     // the readers of the call before are done
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kPlocFinish / 64; k++) { before += k < w ? wsum[k] : 0u; all += wsum[k]; }
    *total = all;
    return before + x - v;
}

// The finisher, in two kernels of one workgroup each, continues what `k` device-wide iterations left and runs the rule until one cluster
// is left; at most I + clog2(n) iterations are run in all.
// k_ploc_shrink: while C > 1024 an iteration walks the two buffers in global memory, 1024 positions at a time (the order between its
// steps is the workgroup's barrier): slow, but bounded.  It leaves the buffer in use, C and t in state[4 .. 6].
__global__ __launch_bounds__(kPlocFinish) void k_ploc_shrink(Ploc p, int k) {
    __shared__ uint32_t wsum[kPlocFinish / 64];
    if (!resolve(p)) return;
    const int tid = threadIdx.x, I = ploc_nn_iterations(p.n), most = I + clog2(p.n);
    const int D = p.depth_limit ? p.depth_limit : kMaxDepth;
    int cur = k & 1, C = p.state[2 * cur], t = p.state[2 * cur + 1];
    PlocCluster *in = ploc_buffer(p, cur), *out = ploc_buffer(p, cur ^ 1);
    if (tid == 0) { p.state[4] = cur; p.state[5] = C; p.state[6] = t; }
    while (C > kPlocFinish && t < most) {                // every value in the condition is uniform over the block
        const int hcap = D - clog2(C);
        for (int i = tid; i < C; i += kPlocFinish) p.nn[i] = t >= I ? ploc_forced(i, C) : ploc_choose(i, C, p.radius, hcap, in);
        __threadfence_block();
        __syncthreads();
        int leaders = 0, survivors = 0;
        for (int c0 = 0; c0 < C; c0 += kPlocFinish) {
            const int i = c0 + tid;
            int j = -1;
            uint32_t total;
            const uint32_t role = i < C ? ploc_role(i, p.nn, &j) : 0u;
            const uint32_t before = ploc_scan(role, &total, wsum);
            if (role & 1u) {
                const bool lead = (role >> 16) != 0u;
                out[survivors + (int)(before & 0xFFFFu)] =
                    ploc_survivor(p, lead, (C - 2) - (leaders + (int)(before >> 16)), in[i], in[lead ? j : i]);
            }
            leaders += (int)(total >> 16); survivors += (int)(total & 0xFFFFu);
        }
        __threadfence_block();
        __syncthreads();
        PlocCluster* const was = in;
        in = out; out = was;
        cur ^= 1; C -= leaders; t++;
        if (tid == 0) { p.state[4] = cur; p.state[5] = C; p.state[6] = t; }    // the hand-over, kept current
    }
}

// k_ploc_finish: the at most 1024 clusters k_ploc_shrink left stay in LDS to the end; info[7] = the iterations run.
__global__ __launch_bounds__(kPlocFinish) void k_ploc_finish(Ploc p) {
    __shared__ float sb[6 * kPlocFinish];
    __shared__ int sh[kPlocFinish], sid[kPlocFinish], snn[kPlocFinish];
    __shared__ uint32_t wsum[kPlocFinish / 64];
    if (!resolve(p)) return;
    const int tid = threadIdx.x, I = ploc_nn_iterations(p.n), most = I + clog2(p.n);
    const int D = p.depth_limit ? p.depth_limit : kMaxDepth;
    int C = min(p.state[5], kPlocFinish), t = p.state[6];
    if (tid < C) {
        const PlocCluster c = ploc_buffer(p, p.state[4])[tid];
        for (int a = 0; a < 6; a++) sb[a * kPlocFinish + tid] = c.box[a];
        sh[tid] = c.h; sid[tid] = c.id;
    }
    __syncthreads();
    while (C > 1 && t < most) {                          // uniform over the block
        if (tid < C) snn[tid] = t >= I ? ploc_forced(tid, C) : ploc_choose(tid, C, p.radius, D - clog2(C), sb, kPlocFinish, 1, sh, 0);
        __syncthreads();
        int j = -1;
        uint32_t total;
        const uint32_t role = tid < C ? ploc_role(tid, snn, &j) : 0u;
        const bool lead = (role >> 16) != 0u;
        PlocCluster a, b;
        if (role & 1u) {
            const int jj = lead ? j : tid;
            for (int k = 0; k < 6; k++) { a.box[k] = sb[k * kPlocFinish + tid]; b.box[k] = sb[k * kPlocFinish + jj]; }
            a.id = sid[tid]; a.h = sh[tid]; b.id = sid[jj]; b.h = sh[jj];
        }
        const uint32_t before = ploc_scan(role, &total, wsum);        // its barriers stand between the reads above and the writes below
        if (role & 1u) {
            const int q = (int)(before & 0xFFFFu);
            const PlocCluster c = ploc_survivor(p, lead, (C - 2) - (int)(before >> 16), a, b);
            for (int k = 0; k < 6; k++) sb[k * kPlocFinish + q] = c.box[k];
            sid[q] = c.id; sh[q] = c.h;
        }
        __syncthreads();
        C -= (int)(total >> 16);
        t++;
    }
    if (tid == 0) p.info[kInfoIterations] = t;
}
