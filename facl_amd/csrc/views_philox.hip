// The 10 views of a batch of clips with COUNTER-BASED draws (--view_rng philox): no host draw per clip, no host mask
// loop, two launches per batch.  Same views as csrc/views.hip (cn3D_data_set.py:285-350 get_data_train, :654-663,
// :708-713, :734-749, :767-778) and the same arithmetic -- only the random numbers come from Philox4x32-10 instead of
// NumPy's stream, so a clip's views depend on (seed, epoch, dataset index of the clip) and on nothing else: not on its
// position in the batch, the batch size or the number of ranks.
//
// Draw recipe (restated in NumPy by facl_amd/philox.py, which the tests hold this file to):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (point n in 0..511, slot, clip id, epoch)           -> four 32-bit words w0..w3
//   rows    slot 0: views 0,1,2,3 = w0..w3; slot 1: views 4,5,6,7; slot 2: views 8,9 = w0,w1.
//           row = (uint64(w) * count) >> 32 in [0, count) of the view's source cloud (views 6, 7: of the list of rows
//           whose channel 4 / 7 is non-zero, compacted by k_temporal_rows)
//   jitter  slot 3 + 3*j + d (j = jitter slot 0..6 of views.hip, d = xyz): u1 = (w0 + 1) * 2^-32 in (0, 1],
//           u2 = w1 * 2^-32 in [0, 1), z = sqrt(-2 log u1) * cos(2 pi u2) in fp64, then clip(0.01 z, -0.05, 0.05)
//   angle k (k = 0, 1; views 4, 5): counter (0, 24 + k, clip id, epoch), u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53,
//           angle = (u - 0.5) * pi * 0.8, cos / sin in fp64
// Arithmetic: k_build_views' dtype walk -- jitter in fp64 written back in the source dtype, mirror / rotation on float32.
#include "common.h"

namespace {

constexpr int NV = 10, NP = 512;          // views, points per view
constexpr int TR_THREADS = 256;           // k_temporal_rows: 4 waves, 256 rows per pass

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

// meta (B, 9) int32 per clip: row offset of the four source clouds in src, their row counts, the clip's dataset index
constexpr int META = 9;

// one workgroup per clip: the rows of its point cloud whose channel 4 / channel 7 is non-zero, in row order, written to
// list[0][base0 + k] / list[1][base0 + k] (k < count); counts (B, 2).  A zero count raises err (the views must not be used).
template <typename S>
__global__ __launch_bounds__(TR_THREADS) void k_temporal_rows(const S* __restrict__ src, int C, int rows,
                                                              const int* __restrict__ meta, int* __restrict__ list,
                                                              int* __restrict__ counts, int* __restrict__ err) {
    __shared__ int wtot[2][TR_THREADS / FACL_WAVE];
    const int b = blockIdx.x, t = threadIdx.x, w = t / FACL_WAVE;
    const int base = meta[b * META], P = meta[b * META + 4];
    int run4 = 0, run7 = 0;                                       // rows kept so far (uniform across the block)
    const unsigned long long below = lanemask_lt();
    for (int c = 0; c < P; c += TR_THREADS) {
        const int i = c + t;
        bool nz4 = false, nz7 = false;
        if (i < P) {
            const S* r = src + (size_t)(base + i) * C;
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
        if (nz4) list[base + off4 + __popcll(m4 & below)] = base + i;
        if (nz7) list[(size_t)rows + base + off7 + __popcll(m7 & below)] = base + i;
        run4 += tot4; run7 += tot7;
        __syncthreads();                                          // wtot is rewritten by the next pass
    }
    if (t == 0) {
        counts[b * 2] = run4;
        counts[b * 2 + 1] = run7;
        if (run4 == 0 || run7 == 0) *err = 1;
    }
}

// block = one (clip, view); thread = one point.  idx_out (B, 10, 512), optional: the absolute source row of every point.
template <typename S>
__global__ __launch_bounds__(NP) void k_build_views_philox(const S* __restrict__ src, int C, int rows,
                                                           const int* __restrict__ meta, const int* __restrict__ list,
                                                           const int* __restrict__ counts, uint32_t k0, uint32_t k1,
                                                           uint32_t epoch, int B, float* __restrict__ out,
                                                           int* __restrict__ idx_out) {
    const int b = blockIdx.x / NV, v = blockIdx.x % NV, n = threadIdx.x;
    const int* m = meta + b * META;
    const uint32_t cid = (uint32_t)m[8];
    float* dst = out + (((size_t)v * B + b) * NP + n) * 4;
    // source cloud of each view: points 0,0 | key 1,1 | points 0,0 | temporal lists | res1 2 | res2 3
    const int src_of = v < 2 ? 0 : (v < 4 ? 1 : (v < 8 ? 0 : v - 6));
    const u32x4 rw = philox4x32_10((uint32_t)n, (uint32_t)(v >> 2), cid, epoch, k0, k1);
    const uint32_t word = rw.w[v & 3];
    int row;
    if (v == 6 || v == 7) {
        const int cnt = counts[b * 2 + (v - 6)];
        if (cnt == 0) {                                          // no row to draw from: err is set, the views are void
            *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx_out) idx_out[((size_t)b * NV + v) * NP + n] = -1;
            return;
        }
        row = list[(size_t)(v - 6) * rows + m[0] + draw_row(word, cnt)];
    } else {
        row = m[src_of] + draw_row(word, m[4 + src_of]);
    }
    if (idx_out) idx_out[((size_t)b * NV + v) * NP + n] = row;
    const S* r = src + (size_t)row * C;
    const int c3 = v == 6 ? 4 : (v == 7 ? 7 : 3);
    S x[3] = {r[0], r[1], r[2]};
    const S w = r[c3];
    float o[4];
    o[3] = (float)w;
    auto z = [&](int slot, int d) -> double {                  // standard normal of jitter slot `slot`, coordinate d
        const u32x4 q = philox4x32_10((uint32_t)n, (uint32_t)(3 + 3 * slot + d), cid, epoch, k0, k1);
        const double u1 = ((double)q.w[0] + 1.0) * 0x1p-32, u2 = (double)q.w[1] * 0x1p-32;
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
        const u32x4 q = philox4x32_10(0u, (uint32_t)(24 + (v - 4)), cid, epoch, k0, k1);
        const double u = ((double)(q.w[0] >> 5) * 67108864.0 + (double)(q.w[1] >> 6)) * 0x1p-53;
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

}  // namespace

template <typename S>
static int launch_temporal_rows(const S* src, int64_t rows, int C, const int32_t* meta, int B, int32_t* list,
                                int32_t* counts, int32_t* err, void* stream) {
    if (!src || !meta || !list || !counts || !err) return FACL_E_NULL;
    if (B < 1 || rows < 1 || rows > INT32_MAX / 2 || C < 8 || B > (1 << 20)) return FACL_E_SHAPE;
    hipLaunchKernelGGL((k_temporal_rows<S>), dim3(B), dim3(TR_THREADS), 0, (hipStream_t)stream, src, C, (int)rows, meta,
                       list, counts, err);
    return facl_launch_status();
}

template <typename S>
static int launch_views_philox(const S* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                               const int32_t* counts, int64_t seed, int epoch, int B, float* out, int32_t* idx_out,
                               void* stream) {
    if (!src || !meta || !list || !counts || !out) return FACL_E_NULL;
    if (B < 1 || rows < 1 || rows > INT32_MAX / 2 || C < 8 || B > (1 << 20)) return FACL_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) % 16) return FACL_E_ALIGN;
    const uint64_t s = (uint64_t)seed;
    hipLaunchKernelGGL((k_build_views_philox<S>), dim3(B * NV), dim3(NP), 0, (hipStream_t)stream, src, C, (int)rows, meta,
                       list, counts, (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), (uint32_t)epoch, B, out, idx_out);
    return facl_launch_status();
}

extern "C" int facl_views_temporal_rows_f32(const float* src, int64_t rows, int C, const int32_t* meta, int B,
                                            int32_t* list, int32_t* counts, int32_t* err, void* stream) {
    return launch_temporal_rows<float>(src, rows, C, meta, B, list, counts, err, stream);
}

extern "C" int facl_views_temporal_rows_f64(const double* src, int64_t rows, int C, const int32_t* meta, int B,
                                            int32_t* list, int32_t* counts, int32_t* err, void* stream) {
    return launch_temporal_rows<double>(src, rows, C, meta, B, list, counts, err, stream);
}

extern "C" int facl_build_views_philox_f32(const float* src, int64_t rows, int C, const int32_t* meta,
                                           const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                           float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, out, idx_out, stream);
}

extern "C" int facl_build_views_philox_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                           const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                           float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, out, idx_out, stream);
}
