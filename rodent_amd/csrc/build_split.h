// build_split.h -- stage 9 of the device BVH builder (included by bvh_build.hip after build_treelet.h).
#pragma once
// ---- 9. triangle pre-splitting (Karras & Aila 2013, section 5; the rules in include/rodent_build.h) -----------------------------
// Per triangle: k_split_boxes (box, frame partials, flags), k_split_frame, k_priority (p and its max), k_weights (w and W), k_allot
// (s and the block totals of s + 1), a scan, k_split (the pieces, in the triangle's slot range), a scan of the pieces made (n' in
// info[4]), k_refs (the references in order, their Morton points and point bounds).  Then launch_tree and the tails over n'.
// a cut loop takes at most 2 * 63 + 1 cuts and emits plus 3 * 1023 one-sided cuts (each removes a plane)
constexpr int kSplitSteps = 4096;
enum { kInfoRefs = 4, kInfoSplit = 5, kInfoUnmade = 6 };

// Canonical vertices of triangle t (x + 0: no -0), as rows V[vertex][axis]; returns the error flags.
__device__ __forceinline__ int load_canon(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int t,
                                          float V[3][3], int* info) {
    float3 v[3]; int geom;
    const int flags = load_triangle(vertices, nv, indices, t, v, &geom, info);
    for (int k = 0; k < 3; k++) { V[k][0] = canon(v[k].x); V[k][1] = canon(v[k].y); V[k][2] = canon(v[k].z); }
    return flags;
}

__global__ __launch_bounds__(kBlock) void k_split_boxes(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                        int n, float* __restrict__ tbox, float* __restrict__ partial, int* info) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        float3 v[3]; int geom;
        load_triangle(vertices, nv, indices, t, v, &geom, info);
        float b[6];
        triangle_box(v, b);
        for (int k = 0; k < 6; k++) tbox[6 * (size_t)t + k] = b[k];
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b[2 * a]); hi[a] = fmaxf(hi[a], b[2 * a + 1]); }
    }
    block_bounds(lo, hi, partial + 6 * blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_split_frame(const float* __restrict__ partial, int blocks, float* __restrict__ sframe) {
    const float (*red)[kBlock] = reduce_partials(partial, blocks);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float step = (red[3 + a][0] - red[a][0]) * 0x1p-10f;
        sframe[a] = red[a][0];
        sframe[3 + a] = (step > 0.0f && isfinite(step)) ? step : 0.0f;     // 0: the axis has no planes
    }
}

// The plane of box b: the coarsest grid plane strictly inside it, ties to x, y, z.  Returns its level (-1: none), *axis and *x.
// Per axis two binary searches over the monotone positions lo + (float)c * step give the planes strictly inside, c in [cmin, cmax];
// the coarsest of them keeps the bits above the highest bit where cmin - 1 and cmax differ.
__device__ __forceinline__ int find_plane(const float* __restrict__ sframe, const float b[6], int* axis, float* x) {
    int best = -1;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = sframe[a], step = sframe[3 + a];
        if (!(step > 0.0f)) continue;
        int c0 = 1, h0 = 1024, c1 = 1, h1 = 1024;        // first c with pos > b_lo, first c with pos >= b_hi (1024: none)
        for (int it = 0; it < 10; it++) {
            const int m0 = (c0 + h0) >> 1, m1 = (c1 + h1) >> 1;
            if (c0 < h0) { if (lo + (float)m0 * step > b[2 * a]) h0 = m0; else c0 = m0 + 1; }
            if (c1 < h1) { if (lo + (float)m1 * step >= b[2 * a + 1]) h1 = m1; else c1 = m1 + 1; }
        }
        const int cmin = c0, cmax = c1 - 1;
        if (cmin > cmax) continue;
        const int level = 31 - __clz((cmin - 1) ^ cmax), c = (cmax >> level) << level;
        if (level > best) { best = level; *axis = a; *x = lo + (float)c * step; }
    }
    return best;
}

__device__ __forceinline__ float pick(const float v[3], int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// The SBVH reference split of the triangle V's piece B at plane (axis, x) into boxes L and R (empty: lo > hi on some axis).  Fully
// unrolled, the axis selected by compares: no runtime-indexed private array.
__device__ __forceinline__ void cut(const float V[3][3], const float B[6], int axis, float x, float L[6], float R[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) { L[k] = (k & 1) ? -INFINITY : INFINITY; R[k] = L[k]; }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float* P = V[i];
        const float* Q = V[(i + 1) % 3];
        const float pa = pick(P, axis), qa = pick(Q, axis);
#pragma unroll
        for (int b = 0; b < 3; b++) {
            if (pa <= x) { L[2 * b] = fminf(L[2 * b], P[b]); L[2 * b + 1] = fmaxf(L[2 * b + 1], P[b]); }
            if (pa >= x) { R[2 * b] = fminf(R[2 * b], P[b]); R[2 * b + 1] = fmaxf(R[2 * b + 1], P[b]); }
        }
        if ((pa < x && qa > x) || (pa > x && qa < x)) {
            const float t = __fdiv_rn(x - pa, qa - pa);
#pragma unroll
            for (int b = 0; b < 3; b++) {
                float lo = x, hi = x;
                if (b != axis) {
                    const float y = P[b] + t * (Q[b] - P[b]);
                    const float g = fmaxf(fmaxf(fabsf(P[b]), fabsf(Q[b])) * 0x1p-19f, 0x1p-126f);
                    lo = fmaxf(y - g, fminf(P[b], Q[b]));
                    hi = fminf(y + g, fmaxf(P[b], Q[b]));
                }
                L[2 * b] = fminf(L[2 * b], lo); L[2 * b + 1] = fmaxf(L[2 * b + 1], hi);
                R[2 * b] = fminf(R[2 * b], lo); R[2 * b + 1] = fmaxf(R[2 * b + 1], hi);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 3; b++) {
        L[2 * b] = fmaxf(L[2 * b], B[2 * b]); L[2 * b + 1] = fminf(L[2 * b + 1], B[2 * b + 1]);
        R[2 * b] = fmaxf(R[2 * b], B[2 * b]); R[2 * b + 1] = fminf(R[2 * b + 1], B[2 * b + 1]);
        if (b == axis) { L[2 * b + 1] = fminf(L[2 * b + 1], x); R[2 * b] = fmaxf(R[2 * b], x); }
    }
}

__device__ __forceinline__ bool box_empty(const float b[6]) { return b[0] > b[1] || b[2] > b[3] || b[4] > b[5]; }
__device__ __forceinline__ float longest(const float b[6]) { return fmaxf(fmaxf(b[1] - b[0], b[3] - b[2]), b[5] - b[4]); }

__global__ __launch_bounds__(kBlock) void k_priority(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices,
                                                     int n, const float* __restrict__ tbox, const float* __restrict__ sframe,
                                                     float* __restrict__ prio, uint32_t* pmax) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    float p = 0.0f;
    if (t < n) {
        float V[3][3];
        if (!load_canon(vertices, nv, indices, t, V, nullptr)) {
            float b[6];
            for (int k = 0; k < 6; k++) b[k] = tbox[6 * (size_t)t + k];
            int axis; float x;
            const int level = find_plane(sframe, b, &axis, &x);
            if (level >= 0) {
                const float ex = V[1][0] - V[0][0], ey = V[1][1] - V[0][1], ez = V[1][2] - V[0][2];
                const float fx = V[2][0] - V[0][0], fy = V[2][1] - V[0][1], fz = V[2][2] - V[0][2];
                const float nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
                const float excess = fmaxf(0.0f, half_area(b) - 0.5f * ((fabsf(nx) + fabsf(ny)) + fabsf(nz)));
                p = __fsqrt_rn((float)(1 << level) * excess);
                if (!isfinite(p)) p = 0.0f;
            }
        }
        prio[t] = p;
    }
    float m = p;
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (lane_id() == 0) atomicMax(pmax, __float_as_uint(m));
}

__global__ __launch_bounds__(kBlock) void k_weights(const float* __restrict__ prio, int n, const uint32_t* __restrict__ pmax,
                                                    uint32_t* __restrict__ w, unsigned long long* wsum) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const float top = __uint_as_float(*pmax);
    uint32_t wt = 0;
    if (t < n) {
        if (top > 0.0f) wt = (uint32_t)floorf(__fdiv_rn(prio[t], top) * 65536.0f);
        w[t] = wt;
    }
    uint32_t sum = wt;                                   // at most 64 * 65536 per wave
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane_id() == 0 && sum) atomicAdd(wsum, (unsigned long long)sum);
}

__global__ __launch_bounds__(kBlock) void k_allot(const uint32_t* __restrict__ w, int n, long long budget, int max_pieces,
                                                  const unsigned long long* __restrict__ wsum, uint32_t* __restrict__ s,
                                                  uint32_t* __restrict__ blocktot, int* info) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long W = *wsum;
    uint32_t st = 0;
    if (t < n) {
        if (W) st = (uint32_t)std::min((unsigned long long)(max_pieces - 1), ((unsigned long long)w[t] * (unsigned long long)budget) / W);
        s[t] = st;
    }
    const uint64_t split = __ballot(st > 0);
    if (lane_id() == 0 && split) atomicAdd(&info[kInfoSplit], (int)__popcll(split));
    uint32_t total;
    block_scan(t < n ? st + 1 : 0u, &total);
    if (threadIdx.x == 0) blocktot[blockIdx.x] = total;
}

// One thread per triangle cuts it into at most s + 1 pieces inside its slot range [start, start + s]: final pieces from the front,
// pending ones (box + splits) on a stack growing down from the back.  Every pending piece ends as at least one final piece and every
// cut spends a split, so (final pieces) + (pending pieces) <= s + 1: the two ends never meet.
__global__ __launch_bounds__(kBlock) void k_split(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int n,
                                                  const float* __restrict__ tbox, const float* __restrict__ sframe,
                                                  const uint32_t* __restrict__ s, const uint32_t* __restrict__ blockoff,
                                                  float* __restrict__ pbox, int* __restrict__ pk, uint32_t* __restrict__ start,
                                                  uint32_t* __restrict__ made, uint32_t* __restrict__ blockmade, int* info) {
    __shared__ uint32_t block_made;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int st = t < n ? (int)s[t] : 0;
    uint32_t total;
    const uint32_t first = blockoff[blockIdx.x] + block_scan(t < n ? (uint32_t)st + 1 : 0u, &total);
    if (threadIdx.x == 0) block_made = 0;
    __syncthreads();
    int out = 1;
    if (t < n && st > 0) {
        float V[3][3], cb[6];
        load_canon(vertices, nv, indices, t, V, nullptr);
        for (int k = 0; k < 6; k++) cb[k] = tbox[6 * (size_t)t + k];
        int k = st, sp = 0, unmade = 0;
        out = 0;
        for (int step = 0; step < kSplitSteps; step++) {
            int axis = 0; float x = 0.0f;
            bool final = k == 0 || find_plane(sframe, cb, &axis, &x) < 0;
            if (!final) {
                float L[6], R[6];
                cut(V, cb, axis, x, L, R);
                const bool le = box_empty(L), re = box_empty(R);
                if (le && re) {
                    final = true;
                } else if (le || re) {                   // the piece lies on one side: it takes that side's box and keeps its splits
                    for (int j = 0; j < 6; j++) cb[j] = le ? R[j] : L[j];
                    continue;
                } else {
                    const float el = longest(L), er = longest(R);
                    const float q = __fdiv_rn((float)(k - 1) * el, el + er);
                    const int kl = (int)fminf(fmaxf(floorf(q + 0.5f), 0.0f), (float)(k - 1));
                    const size_t slot = first + (size_t)(st - sp);
                    for (int j = 0; j < 6; j++) pbox[6 * slot + j] = R[j];
                    pk[slot] = k - 1 - kl;
                    sp++;
                    for (int j = 0; j < 6; j++) cb[j] = L[j];
                    k = kl;
                    continue;
                }
            }
            unmade += k;
            const size_t slot = first + (size_t)out;
            for (int j = 0; j < 6; j++) pbox[6 * slot + j] = canon(cb[j]);
            out++;
            if (sp == 0) break;
            sp--;
            const size_t top = first + (size_t)(st - sp);
            for (int j = 0; j < 6; j++) cb[j] = pbox[6 * top + j];
            k = pk[top];
        }
        if (unmade) atomicAdd(&info[kInfoUnmade], unmade);
    }
    if (t < n) { start[t] = first; made[t] = (uint32_t)out; atomicAdd(&block_made, (uint32_t)out); }
    __syncthreads();
    if (threadIdx.x == 0) blockmade[blockIdx.x] = block_made;
}

// References in order: per triangle its pieces (or, uncut, its box and vertex sum), their Morton points and the block's point bounds.
__global__ __launch_bounds__(kBlock) void k_refs(const float4* __restrict__ vertices, int nv, const int4* __restrict__ indices, int n,
                                                 const float* __restrict__ tbox, const uint32_t* __restrict__ s,
                                                 const uint32_t* __restrict__ start, const uint32_t* __restrict__ made,
                                                 const uint32_t* __restrict__ blockoff, const float* __restrict__ pbox,
                                                 float* __restrict__ refbox, int* __restrict__ reftri, float4* __restrict__ cent,
                                                 float* __restrict__ kpartial) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    const uint32_t dst = blockoff[blockIdx.x] + block_scan(t < n ? made[t] : 0u, &total);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (t < n) {
        if (s[t] == 0) {
            float3 v[3]; int geom;
            load_triangle(vertices, nv, indices, t, v, &geom, nullptr);
            const float c[3] = {(v[0].x + v[1].x) + v[2].x, (v[0].y + v[1].y) + v[2].y, (v[0].z + v[1].z) + v[2].z};
            for (int k = 0; k < 6; k++) refbox[6 * (size_t)dst + k] = tbox[6 * (size_t)t + k];
            reftri[dst] = t;
            cent[dst] = make_float4(c[0], c[1], c[2], 0.0f);
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
        } else {
            const uint32_t count = made[t];
            for (uint32_t j = 0; j < count; j++) {
                const float* b = pbox + 6 * ((size_t)start[t] + j);
                float c[3];
                for (int a = 0; a < 3; a++) c[a] = (b[2 * a] + b[2 * a + 1]) * 1.5f;
                for (int k = 0; k < 6; k++) refbox[6 * ((size_t)dst + j) + k] = b[k];
                reftri[dst + j] = t;
                cent[dst + j] = make_float4(c[0], c[1], c[2], 0.0f);
                for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
            }
        }
    }
    block_bounds(lo, hi, kpartial + 6 * blockIdx.x);
}
