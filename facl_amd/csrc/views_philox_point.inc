// The per-point half of the counter-based views, shared by csrc/views_philox.hip (a packed batch from disk) and
// csrc/views_resident.hip (clips selected by index out of a pool resident in device memory): the Philox4x32-10 block, the
// draw recipe (which word of which counter picks the row of a view's point, the Box-Muller jitter, the rotation angle) and
// the dtype walk of the arithmetic.  The two kernels differ only in how a drawn position becomes a row of their source
// array; everything a view's VALUES depend on lives here, once, so the two paths cannot drift apart (their views are
// required to be equal bit for bit).  Include inside an anonymous namespace, after common.h.  The recipe is written out
// in the header of views_philox.hip and restated in NumPy by facl_amd/philox.py.
//
// G views of P points per clip (both run-time arguments): view v is of KIND k = v % 10 (the reference's ten views) in
// ROUND r = v / 10; every draw slot of round r is the kind's slot + 32 * r, the point index n runs over 0..P-1.

constexpr int KINDS = 10;                 // the reference's ten views = the kinds of a round
constexpr int ROUND_SLOTS = 32;           // counter slots per round (26 in use: rows 0..2, jitter 3..23, angles 24, 25)
constexpr int CHUNK = 512;                // points per workgroup at most (the reference's cloud: one workgroup per view)
constexpr int G_MAX = 64, P_MIN = 64, P_MAX = 4096;
constexpr int TR_THREADS = 256;           // temporal-row compaction: 4 waves, 256 rows per pass

struct u32x4 { uint32_t w[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ int draw_row(uint32_t w, int count) {
    return (int)(((unsigned long long)w * (unsigned long long)(uint32_t)count) >> 32);
}

__device__ __forceinline__ double jit(double n) {          // np.clip(0.01 * n, -0.05, 0.05)
    const double v = 0.01 * n;
    return v < -0.05 ? -0.05 : (v > 0.05 ? 0.05 : v);
}

// what a (clip, view, point) draws with: the key, the clip's dataset index and the epoch
struct ViewDraw { uint32_t k0, k1, cid, epoch; };

__device__ __forceinline__ ViewDraw view_draw(int64_t seed, uint32_t cid, int epoch) {
    const uint64_t s = (uint64_t)seed;
    return {(uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), cid, (uint32_t)epoch};
}

// the domain of (G, P): 1..64 views; 64..4096 points in whole waves (the upper bound is the grouping limit)
static inline bool views_gp_ok(int G, int P) {
    return G >= 1 && G <= G_MAX && P >= P_MIN && P <= P_MAX && P % FACL_WAVE == 0;
}

// launch geometry: workgroups of (clip, view, chunk of up to 512 points), `threads` points each
struct ViewGrid { int threads, chunks; };
static inline ViewGrid view_grid(int P) {
    const int threads = P < CHUNK ? P : CHUNK;
    return {threads, (P + threads - 1) / threads};
}

// where a workgroup stands: clip b of the batch, view v = kind k of round `round`, point n (n >= P: nothing to do)
struct ViewAt { int b, v, k, slot0, n; };

__device__ __forceinline__ ViewAt view_at(int G, int chunks) {
    const int c = (int)blockIdx.x % chunks, bv = (int)blockIdx.x / chunks;
    const int v = bv % G;
    return {bv / G, v, v % KINDS, ROUND_SLOTS * (v / KINDS), c * (int)blockDim.x + (int)threadIdx.x};
}

// source cloud of each kind: points 0,0 | key 1,1 | points 0,0 | temporal lists (of cloud 0) | res1 2 | res2 3
__device__ __forceinline__ int view_source(int k) { return k < 2 ? 0 : (k < 4 ? 1 : (k < 8 ? 0 : k - 6)); }

// the 32-bit word that picks the source row of point n of a view of kind k: draw_row(word, count) in [0, count)
__device__ __forceinline__ uint32_t view_row_word(const ViewDraw& q, int k, int slot0, int n) {
    const u32x4 rw = philox4x32_10((uint32_t)n, (uint32_t)(slot0 + (k >> 2)), q.cid, q.epoch, q.k0, q.k1);
    return rw.w[k & 3];
}

__device__ __forceinline__ void view_void(float* dst) {    // a view that cannot be drawn: zeros
    *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// point n of a view of kind v (slots from slot0 = 32 * round) from its source row r (>= 8 channels): jitter in fp64
// written back in the source dtype, mirror / rotation on float32, channel select; one float4 store to dst
template <typename S>
__device__ __forceinline__ void view_point(const S* __restrict__ r, const ViewDraw& q, int v, int slot0, int n,
                                           float* __restrict__ dst) {
    const uint32_t cid = q.cid, epoch = q.epoch, k0 = q.k0, k1 = q.k1;
    const int c3 = v == 6 ? 4 : (v == 7 ? 7 : 3);
    S x[3] = {r[0], r[1], r[2]};
    const S w = r[c3];
    float o[4];
    o[3] = (float)w;
    auto z = [&](int slot, int d) -> double {                  // standard normal of jitter slot `slot`, coordinate d
        const u32x4 p = philox4x32_10((uint32_t)n, (uint32_t)(slot0 + 3 + 3 * slot + d), cid, epoch, k0, k1);
        const double u1 = ((double)p.w[0] + 1.0) * 0x1p-32, u2 = (double)p.w[1] * 0x1p-32;
        return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    };
    auto jitter_into_src = [&](int slot) {
#pragma unroll
        for (int d = 0; d < 3; ++d) x[d] = (S)((double)x[d] + jit(z(slot, d)));
    };
    if (v == 1 || v == 3) {                                  // jitter, then reverse_transform (:708-713)
        const int s0 = v == 1 ? 0 : 3;
        jitter_into_src(s0);
        float f[3] = {(float)x[0], (float)x[1], (float)x[2]};
        f[0] = -f[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = (float)((double)f[d] + jit(z(s0 + 1, d)));
    } else if (v == 2) {
        jitter_into_src(2);
        o[0] = (float)x[0]; o[1] = (float)x[1]; o[2] = (float)x[2];
    } else if (v == 4 || v == 5) {                           // jitter, then rotate_trans (:734-749)
        jitter_into_src(v == 4 ? 5 : 6);
        const u32x4 p = philox4x32_10(0u, (uint32_t)(slot0 + 24 + (v - 4)), cid, epoch, k0, k1);
        const double u = ((double)(p.w[0] >> 5) * 67108864.0 + (double)(p.w[1] >> 6)) * 0x1p-53;
        const double angle = (u - 0.5) * 3.141592653589793 * 0.8;
        const double c = cos(angle), s = sin(angle);
        const double fx = (double)(float)x[0], fy = (double)(float)x[1], fz = (double)(float)x[2];
        o[0] = (float)(fx * c + fz * (-s));
        o[1] = (float)fy;
        o[2] = (float)(fx * s + fz * c);
    } else {                                                 // raw, temporal, low-resolution views: plain gather
        o[0] = (float)x[0]; o[1] = (float)x[1]; o[2] = (float)x[2];
    }
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
}

// One pass of the ballot / popcount-prefix walk over rows [c, c + TR_THREADS) of a clip's point cloud (P rows of C
// channels at `cloud`): the rows whose channel 4 / channel 7 is non-zero go, in row order, to l4[run4 + ..] / l7[run7 + ..]
// as `bias + row`; run4 / run7 (uniform across the block) advance by the rows kept.  wtot: 2 x (TR_THREADS / FACL_WAVE)
// ints of shared memory.  Every thread of the block calls it (two barriers inside).
template <typename S, typename R>
__device__ __forceinline__ void temporal_rows_pass(const S* __restrict__ cloud, int C, int P, int c, R bias,
                                                   R* __restrict__ l4, R* __restrict__ l7, int& run4, int& run7,
                                                   int (*wtot)[TR_THREADS / FACL_WAVE]) {
    const int t = threadIdx.x, w = t / FACL_WAVE;
    const unsigned long long below = lanemask_lt();
    const int i = c + t;
    bool nz4 = false, nz7 = false;
    if (i < P) {
        const S* r = cloud + (size_t)i * C;
        nz4 = r[4] != (S)0;
        nz7 = r[7] != (S)0;
    }
    const unsigned long long m4 = __ballot(nz4), m7 = __ballot(nz7);
    if (lane_id() == 0) {
        wtot[0][w] = __popcll(m4);
        wtot[1][w] = __popcll(m7);
    }
    __syncthreads();
    int off4 = run4, off7 = run7, tot4 = 0, tot7 = 0;
#pragma unroll
    for (int k = 0; k < TR_THREADS / FACL_WAVE; ++k) {
        if (k < w) { off4 += wtot[0][k]; off7 += wtot[1][k]; }
        tot4 += wtot[0][k]; tot7 += wtot[1][k];
    }
    if (nz4) l4[off4 + __popcll(m4 & below)] = bias + (R)i;
    if (nz7) l7[off7 + __popcll(m7 & below)] = bias + (R)i;
    run4 += tot4; run7 += tot7;
    __syncthreads();                                          // wtot is rewritten by the next pass
}
