// Small fp64 "finalize" kernels between the passes of the train-mode BatchNorm pipeline:
// partial-sum reduction, BN statistics -> (mean, invstd, scale, shift, sign), running-stat update (the arithmetic: bn_consts.h).
#include "bn_consts.h"
#include <stdlib.h>

extern "C" int64_t facl_ws_bytes(void);

namespace {

// part[rows][V] (doubles or floats) -> out[V]  (deterministic: fixed order, no atomics).  Block = 64 columns x 16 row groups;
// blockIdx.y selects a contiguous slice of `rows_per_block` rows and writes row blockIdx.y of `out` (two-level reduction: the
// partial-sum matrices are up to 12 MB and V/64 blocks alone left the kernel latency-bound at ~10 us a call).
template <typename T>
__global__ __launch_bounds__(1024) void k_reduce_rows(const T* __restrict__ part, int rows, int V,
                                                      int rows_per_block, double* __restrict__ out) {
    __shared__ double red[16][64];
    const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int v = blockIdx.x * 64 + col;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    double s0 = 0, s1 = 0;
    if (v < V) {
        int r = r0 + rg;
        for (; r + 16 < r1; r += 32) {
            s0 += (double)part[(size_t)r * V + v];
            s1 += (double)part[(size_t)(r + 16) * V + v];
        }
        if (r < r1) s0 += (double)part[(size_t)r * V + v];
    }
    red[rg][col] = s0 + s1;
    __syncthreads();
    if (rg == 0 && v < V) {
        double t = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][col];
        out[(size_t)blockIdx.y * V + v] = t;
    }
}

// `prev` (or null): `nprev` floats that the INPUT of this layer was computed with -- the (scale | shift) rows of the previous
// layer's constants.  The heavy passes apply the previous layer's ReLU as fmaxf(v, 0), which turns a NaN activation into a clean
// zero, so a NaN / inf there never reaches this layer's sums; the reference's nn.ReLU keeps it and the next convolution spreads it
// over every channel.  A non-finite value in `prev` therefore makes EVERY statistic of this layer NaN (constants, running buffers),
// as the reference's are: the flag travels bnc1 -> bnc2 -> bnc3, and facl_sa_pool (relu_nan) puts it into the features.
// Finite `prev`: nothing changes, bit for bit.
__device__ __forceinline__ bool block_any_nonfinite(const float* __restrict__ prev, int nprev) {
    __shared__ float flag[16];
    float z = 0.f;
    for (int i = threadIdx.x; i < nprev; i += blockDim.x) z = fmaf(prev[i], 0.f, z);      // 0 * finite = +-0; 0 * inf = 0 * NaN = NaN
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
    if ((threadIdx.x & 63) == 0) flag[threadIdx.x >> 6] = z;
    __syncthreads();
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) z += flag[w];
    return !(z == 0.f);
}

// One workgroup: channels strided over the threads; the pieces are bn_consts.h's.  `aamax` (or null): FACL_AMAX_WORDS uint32 that
// receive -- in every one of the FACL_AMAX_SLOTS slots -- the bits of bn_act_bound's maximum over the channels.  `zamax` (or
// null): a buffer the launch zeroes.  `prev`: see block_any_nonfinite.
__global__ __launch_bounds__(1024) void k_bn_finalize(const double* __restrict__ sums, int C, double count,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                      float momentum, float* __restrict__ running_mean,
                                                      float* __restrict__ running_var, float* __restrict__ bnc,
                                                      unsigned* __restrict__ aamax, unsigned* __restrict__ zamax,
                                                      const float* __restrict__ prev, int nprev) {
    float bound = 0.f;
    const bool poisoned = prev ? block_any_nonfinite(prev, nprev) : false;                // uniform over the workgroup
    if (zamax)
        for (int i = threadIdx.x; i < FACL_AMAX_WORDS; i += blockDim.x) zamax[i] = 0u;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        // poisoned: a NaN sum makes the mean and with it every constant NaN (the bound is NaN too and fmaxf drops it: `aamax` then
        // holds 0, a meaningless scale -- harmless, the constants decide)
        const BnStats st = bn_train_stats(poisoned ? __builtin_nan("") : sums[2 * c], sums[2 * c + 1], count, eps);
        const double g = gamma[c], b = beta[c];
        bn_store_consts(bnc, C, c, (float)st.mean, st.mean, st.invstd, g, b, gamma[c]);
        if (running_mean) bn_running_step(running_mean[c], running_var[c], momentum, st.mean, st.var, count);
        bound = fmaxf(bound, bn_act_bound(g, b, st.var, st.invstd, count));
    }
    if (aamax) bn_store_bound_in_slots<false>(bound, aamax);
}

// the wave's maximum RAISED into the slot of `amax` that its global wave id hashes to (one atomic per wave, non-negative floats
// order like unsigned integers; 256-thread workgroups); `any_bad`: the flag word FACL_AMAX_FLAG_WORD raised to NaN bits as well
__device__ __forceinline__ void raise_wave_slot(float m, unsigned* __restrict__ amax, bool any_bad = false) {
    m = bn_wave_max(m);
    if ((threadIdx.x & 63) == 0) {
        const unsigned wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
        atomicMax(amax + (wave & (FACL_AMAX_SLOTS - 1)) * FACL_AMAX_STRIDE, __float_as_uint(m));
        if (any_bad) atomicMax(amax + FACL_AMAX_FLAG_WORD, 0x7FC00000u);
    }
}

// max|x| over the FINITE elements of a contiguous fp32 array, raised into the slots of `amax` (zeroed by the caller, or holding the
// maximum of another tensor that shares the scale).  A NaN / inf element does not enter the maximum -- one inf would otherwise push
// the operand scale of every OTHER row out of the fp16 range (measured: an inf coordinate in one group left the features of all
// other groups 0.37 off) -- it raises the flag word of the buffer instead (a word no consumer of the scale reads: they take the slots).
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ x, long long n, unsigned* __restrict__ amax) {
    float m = 0.f;
    bool bad = false;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float a = fabsf(x[i]);
        const bool fin = a <= 3.4028235e38f;                      // false for inf and NaN
        m = fmaxf(m, fin ? a : 0.f);
        bad |= !fin;
    }
    raise_wave_slot(m, amax, __ballot(bad) != 0ull);
}

// max of relu(scale[c] y[r][c] + shift[c]) over a (R, C) row-major array: the measured activation maximum of an eval-mode
// layer (running statistics give no bound on the data), raised into `amax` like k_absmax (no flag word).  C % 4 == 0.
__global__ __launch_bounds__(256) void k_rows_act_amax(const float* __restrict__ y, long long n4, int C4,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       unsigned* __restrict__ amax) {
    float m = 0.f;
    const long long stride = (long long)gridDim.x * 256;
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
    int c4 = (int)(i0 % C4);
    const int dc = (int)(stride % C4);
    for (long long i = i0; i < n4; i += stride, c4 = c4 + dc >= C4 ? c4 + dc - C4 : c4 + dc) {
        const float4 v = reinterpret_cast<const float4*>(y)[i];
        const float4 sc = reinterpret_cast<const float4*>(scale)[c4], sh = reinterpret_cast<const float4*>(shift)[c4];
        m = fmaxf(fmaxf(m, fmaxf(fmaf(sc.x, v.x, sh.x), fmaf(sc.y, v.y, sh.y))), fmaxf(fmaf(sc.z, v.z, sh.z), fmaf(sc.w, v.w, sh.w)));
    }
    raise_wave_slot(m, amax);
}

// Eval mode: the constants from the running statistics.  `prev` (or null): as in k_bn_finalize -- `nprev` floats the layer's input
// depends on (the words of the amax buffer facl_absmax measured x into: its flag word holds NaN bits when x held a NaN / inf); a
// non-finite one makes scale and shift NaN.
__global__ void k_bn_eval_consts(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                 const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                 float* __restrict__ bnc, const float* __restrict__ prev, int nprev) {
    const bool poisoned = prev ? block_any_nonfinite(prev, nprev) : false;               // uniform over the workgroup
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double invstd = 1.0 / sqrt((double)rv[c] + (double)eps);
    bn_store_consts(bnc, C, c, rm[c], (double)rm[c], invstd, poisoned ? __builtin_nan("") : (double)gamma[c], (double)beta[c], gamma[c]);
}

__global__ void k_bn1_sums_from_moments(const double* __restrict__ mom, double count, int D,
                                        const float* __restrict__ W1, const float* __restrict__ b1, int C,
                                        double* __restrict__ sums) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) bn1_moment_sums(mom, count, D, W1, b1, c, sums[2 * c], sums[2 * c + 1]);
}

// The three steps between the input moments and the layer-1 table in ONE single-wave launch (training, C = 64): the sums of
// k_bn1_sums_from_moments, the constants / running statistics / activation bound of k_bn_finalize and the folded table of k_l1tab,
// composed of the same pieces, so every output is bit-identical to the three-launch chain (2 launches fewer per step).
__global__ __launch_bounds__(64) void k_sa_bn1_chain(const double* __restrict__ mom, double count, int D,
                                                     const float* __restrict__ W1, const float* __restrict__ b1,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     float momentum, float* __restrict__ running_mean,
                                                     float* __restrict__ running_var, double* __restrict__ sums,
                                                     float* __restrict__ bnc, unsigned* __restrict__ aamax, float* __restrict__ tab) {
    constexpr int C = 64;
    const int c = threadIdx.x;
    double su, sq;
    bn1_moment_sums(mom, count, D, W1, b1, c, su, sq);
    sums[2 * c] = su;
    sums[2 * c + 1] = sq;
    const BnStats st = bn_train_stats(su, sq, count, eps);
    const double g = gamma[c], b = beta[c];
    const BnAffine a = bn_store_consts(bnc, C, c, (float)st.mean, st.mean, st.invstd, g, b, gamma[c]);
    if (running_mean) bn_running_step(running_mean[c], running_var[c], momentum, st.mean, st.var, count);
    if (aamax) bn_store_bound_in_slots<true>(bn_act_bound(g, b, st.var, st.invstd, count), aamax);
    l1tab_row(W1, b1, D, c, a.scale, a.shift, tab);
}

// The folded layer-1 table (l1tab_row) for given constants (null: scale 1, shift 0); one wave, thread = channel.
// `xamax` -> `a1amax` (both or neither): with X = max|x| over all coordinates (facl_absmax), |a1_c| <= X sum_i |w'_ci| + |b'_c|:
// the bound of the layer-1 activation for eval-mode constants (train mode takes BatchNorm's own bound, facl_bn_finalize).
__global__ void k_l1tab(const float* __restrict__ W1, const float* __restrict__ b1, int D,
                        const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ tab,
                        const unsigned* __restrict__ xamax, unsigned* __restrict__ a1amax) {
    const int c = threadIdx.x;
    const L1Row r = l1tab_row(W1, b1, D, c, scale ? scale[c] : 1.0f, shift ? shift[c] : 0.0f, tab);
    if (a1amax) {
        const float X = __uint_as_float(amax_bits(xamax));
        // 1.001: covers the fp32 roundings of the sum and of the (at most 8-term) layer-1 chain many times over
        bn_store_bound_in_slots<true>(fmaf(r.l1, X, fabsf(r.bias)) * 1.001f, a1amax);
    }
}

}  // namespace

// Two-level reductions start at this many partial rows: below it one workgroup per 64 columns walks them all (raising the
// threshold to 400, the five 384-row GEMM statistics in one launch each, changed nothing: 3.19 vs 3.18 ms per step)
constexpr int REDUCE_MIN_ROWS = 128;

// The partials occupy part[0 : rows*V] of the caller's workspace (facl_ws_bytes); the slice rows go right behind them when
// they fit, else the reduction stays single-level.  `part` IS the workspace base in every caller.
// Two levels are TWO launches.  Folding them into one ("the last workgroup done adds the slices", bit-identical) was measured
// SLOWER on MI355X: 3.22 vs 3.10 ms per step, same box, alternating runs -- 17 reductions per step, ~7 us each.  Handing data
// from many workgroups to one inside a kernel needs a device-scope release / acquire (__threadfence), and with one L2 per XCD
// (8 of them, not coherent with each other) that is an L2 write-back + invalidate -- far dearer than the ~1.5 us a kernel
// boundary costs in graph replay.
int facl_reduce_rows(const double* part, int rows, int V, double* out, hipStream_t st) {
    const int cb = (V + 63) / 64;
    int nb = 1;
    if (rows >= REDUCE_MIN_ROWS && cb < 128) {
        nb = 256 / cb;                                   // ~256 workgroups
        if (nb > rows / 32) nb = rows / 32;              // at least 32 rows (2 per row group) per block
        if (nb < 1) nb = 1;
    }
    const size_t cap = (size_t)facl_ws_bytes() / sizeof(double);
    if (nb > 1 && (size_t)rows * V + (size_t)nb * V <= cap) {
        const int rpb = (rows + nb - 1) / nb;
        nb = (rows + rpb - 1) / rpb;
        double* scratch = const_cast<double*>(part) + (size_t)rows * V;
        hipLaunchKernelGGL(k_reduce_rows<double>, dim3(cb, nb), dim3(1024), 0, st, part, rows, V, rpb, scratch);
        hipLaunchKernelGGL(k_reduce_rows<double>, dim3(cb, 1), dim3(1024), 0, st, (const double*)scratch, nb, V, nb, out);
    } else {
        hipLaunchKernelGGL(k_reduce_rows<double>, dim3(cb, 1), dim3(1024), 0, st, part, rows, V, rows, out);
    }
    return facl_launch_status();
}

// fp32 partial rows (a kernel whose per-workgroup sums are fp32 anyway writes and re-reads half the bytes): part[rows][V]
// floats -> out[V] doubles, rows added in the same fixed order as facl_reduce_rows' single level
int facl_reduce_rows_f32(const float* part, int rows, int V, double* out, hipStream_t st) {
    const int cb = (V + 63) / 64;
    hipLaunchKernelGGL(k_reduce_rows<float>, dim3(cb, 1), dim3(1024), 0, st, part, rows, V, rows, out);
    return facl_launch_status();
}

extern "C" int64_t facl_ws_bytes(void) { return (int64_t)FACL_WS_ROWS * 4608 * sizeof(double); }

extern "C" int facl_bn_finalize_after(const double* sums, int C, double count, const float* gamma, const float* beta,
                                      float eps, float momentum, float* running_mean, float* running_var, float* bnc,
                                      uint32_t* aamax, uint32_t* zamax, const float* prev, int nprev, void* stream) {
    if (!sums || !gamma || !beta || !bnc) return FACL_E_NULL;
    if (C < 1 || count < 1 || (prev && nprev < 1)) return FACL_E_SHAPE;
    const int threads = C >= 1024 ? 1024 : (C + 63) / 64 * 64;
    hipLaunchKernelGGL(k_bn_finalize, dim3(1), dim3(threads), 0, (hipStream_t)stream, sums, C, count, gamma,
                       beta, eps, momentum, running_mean, running_var, bnc, aamax, zamax, prev, nprev);
    return facl_launch_status();
}

extern "C" int facl_bn_finalize(const double* sums, int C, double count, const float* gamma, const float* beta,
                                float eps, float momentum, float* running_mean, float* running_var, float* bnc,
                                uint32_t* aamax, uint32_t* zamax, void* stream) {
    return facl_bn_finalize_after(sums, C, count, gamma, beta, eps, momentum, running_mean, running_var, bnc, aamax, zamax,
                                  nullptr, 0, stream);
}

extern "C" int facl_absmax(const float* x, int64_t n, uint32_t* amax, void* stream) {
    if (!x || !amax) return FACL_E_NULL;
    if (n < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_absmax, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, amax);
    return facl_launch_status();
}

extern "C" int facl_rows_act_amax(const float* y, int64_t R, int C, const float* scale, const float* shift, uint32_t* amax,
                                  void* stream) {
    if (!y || !scale || !shift || !amax) return FACL_E_NULL;
    if (R < 1 || C < 4 || (C & 3)) return FACL_E_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)scale) | ((uintptr_t)shift)) & 15) return FACL_E_ALIGN;
    const long long n4 = (long long)R * (C / 4);
    const int grid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_rows_act_amax, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, n4, C / 4, scale, shift, amax);
    return facl_launch_status();
}

extern "C" int facl_bn_eval_consts_after(int C, const float* gamma, const float* beta, const float* running_mean,
                                         const float* running_var, float eps, float* bnc, const float* prev, int nprev,
                                         void* stream) {
    if (!gamma || !beta || !running_mean || !running_var || !bnc) return FACL_E_NULL;
    if (C < 1 || (prev && nprev < 1)) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_bn_eval_consts, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, C, gamma, beta,
                       running_mean, running_var, eps, bnc, prev, nprev);
    return facl_launch_status();
}

extern "C" int facl_bn_eval_consts(int C, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, float* bnc, void* stream) {
    return facl_bn_eval_consts_after(C, gamma, beta, running_mean, running_var, eps, bnc, nullptr, 0, stream);
}

extern "C" int facl_bn1_sums_from_moments(const double* mom, double count, int D, const float* W1, const float* b1,
                                          double* sums, void* stream) {
    if (!mom || !W1 || !b1 || !sums) return FACL_E_NULL;
    if (D < FACL_SA_D_MIN || D > FACL_SA_D_MAX) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_bn1_sums_from_moments, dim3(1), dim3(64), 0, (hipStream_t)stream, mom, count, D, W1, b1, 64,
                       sums);
    return facl_launch_status();
}

extern "C" int facl_sa_bn1_chain(const double* mom, double count, int D, const float* W1, const float* b1, const float* gamma,
                                 const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                 double* sums, float* bnc, uint32_t* aamax, float* l1tab, void* stream) {
    if (!mom || !W1 || !b1 || !gamma || !beta || !sums || !bnc || !l1tab) return FACL_E_NULL;
    if (D < FACL_SA_D_MIN || D > FACL_SA_D_MAX || count < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_sa_bn1_chain, dim3(1), dim3(64), 0, (hipStream_t)stream, mom, count, D, W1, b1, gamma, beta, eps, momentum,
                       running_mean, running_var, sums, bnc, aamax, l1tab);
    return facl_launch_status();
}

extern "C" int facl_sa_l1tab(const float* W1, const float* b1, int D, const float* scale, const float* shift,
                             float* l1tab, const uint32_t* xamax, uint32_t* a1amax, void* stream) {
    if (!W1 || !b1 || !l1tab || ((xamax == nullptr) != (a1amax == nullptr))) return FACL_E_NULL;
    if (D < FACL_SA_D_MIN || D > FACL_SA_D_MAX) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_l1tab, dim3(1), dim3(64), 0, (hipStream_t)stream, W1, b1, D, scale, shift, l1tab, xamax, a1amax);
    return facl_launch_status();
}

// ================================================================================================
// Closed-form assembly between the backward passes of the SA point-MLP (csrc/sa_bwd.hip), fp64.
namespace {

// G3 = W3^T diag(g) W3,  h3' = W3^T (-(1/P) s3 dbeta3 + g (b3 - mean3)),  g = -(1/P) s3 dgamma3 invstd3
// Workgroup = 64 outputs x 4 channel quarters: thread (output, quarter) adds its 64 channels in order, the quarters meet in LDS and
// are added in quarter order (one fixed order: deterministic).  65 workgroups instead of 17 whole-W3 ones (the 256-term fp64 dots
// of one thread per output were a 14 us serial chain between k_sa_bwd0 and k_sa_bwd1).
__global__ __launch_bounds__(256) void k_sa_bwd_consts3(const double* __restrict__ sums0, const float* __restrict__ bnc3,
                                                        const float* __restrict__ W3, const float* __restrict__ b3,
                                                        double P, float* __restrict__ G3, float* __restrict__ h3) {
    __shared__ double g[256], hc[256];
    __shared__ double red[3][64];
    const int c = threadIdx.x;
    {
        const double mean = bn_row(bnc3, 256, BN_MEAN)[c], inv = bn_row(bnc3, 256, BN_INVSTD)[c], sc = bn_row(bnc3, 256, BN_SCALE)[c];
        const double gg = -(sc * sums0[2 * c + 1] * inv) / P;
        g[c] = gg;
        hc[c] = -(sc * sums0[2 * c]) / P + gg * ((double)b3[c] - mean);
    }
    __syncthreads();
    const int j = threadIdx.x & 63, qt = threadIdx.x >> 6;          // output column, channel quarter
    const int k = blockIdx.x;                                        // 0..63: row k of G3; 64: h3
    double s = 0;
    if (k < 64) {
#pragma unroll 8
        for (int cc = 64 * qt; cc < 64 * qt + 64; ++cc) s += g[cc] * (double)W3[cc * 64 + k] * (double)W3[cc * 64 + j];
    } else {
#pragma unroll 8
        for (int cc = 64 * qt; cc < 64 * qt + 64; ++cc) s += hc[cc] * (double)W3[cc * 64 + j];
    }
    if (qt) red[qt - 1][j] = s;
    __syncthreads();
    if (qt == 0) {
        s += red[0][j]; s += red[1][j]; s += red[2][j];
        if (k < 64) G3[k * 64 + j] = (float)s;
        else h3[j] = (float)s;
    }
}

// bw2 (4,64): dy2 = scale2*dz2 + A + B*(y2 - mean2)
__global__ void k_sa_bwd_consts2(const double* __restrict__ sums1, const float* __restrict__ bnc2, double P,
                                 float* __restrict__ bw2) {
    const int c = threadIdx.x;
    if (c >= 64) return;
    const double inv = bn_row(bnc2, 64, BN_INVSTD)[c], sc = bn_row(bnc2, 64, BN_SCALE)[c];
    bw2[c] = (float)sc;
    bw2[64 + c] = (float)(-sc * sums1[2 * c] / P);
    bw2[128 + c] = (float)(-sc * inv * sums1[2 * c + 1] / P);
    bw2[192 + c] = bn_row(bnc2, 64, BN_MEAN)[c];
}

// ---- the output walk of facl_sa_bwd_final and facl_sa_bwd_final_frozen: one thread per output, five segments -------------------
// dW3[c][k] | (dbeta3, dgamma3[, db3]) of a channel | dW2 | (dbeta2, dgamma2[, db2]) of a channel | layer 1, one channel per thread
enum SaFinalSeg { SA_DW3, SA_BN3, SA_DW2, SA_BN2, SA_L1, SA_FINAL_PAST };
constexpr int SA_N_DW3 = 256 * 64, SA_N_BN3 = 256, SA_N_DW2 = 64 * 64, SA_N_BN2 = 64, SA_N_L1 = 64;
constexpr int SA_FINAL_TOTAL = SA_N_DW3 + SA_N_BN3 + SA_N_DW2 + SA_N_BN2 + SA_N_L1;
// output index o -> its segment, r = the index within it
__device__ __forceinline__ SaFinalSeg sa_final_segment(int o, int& r) {
    r = o;
    if (r < SA_N_DW3) return SA_DW3;
    if ((r -= SA_N_DW3) < SA_N_BN3) return SA_BN3;
    if ((r -= SA_N_BN3) < SA_N_DW2) return SA_DW2;
    if ((r -= SA_N_DW2) < SA_N_BN2) return SA_BN2;
    return (r -= SA_N_BN2) < SA_N_L1 ? SA_L1 : SA_FINAL_PAST;
}
// (dbeta1, dgamma1) of channel c from R1 (FACL_SA_L1_COLS(D),64) = rows sum_p x_d dz1 (d < D), then sum_p dz1 -- the tail of
// facl_sa_bwd2's output: dgamma1 = sum_p dz1 (y1 - mean) invstd with y1 = W1 x + b1; bmm = b1 - mean
struct L1Grads { double dbeta, dgamma; };
__device__ __forceinline__ L1Grads l1_bn_grads(const double* __restrict__ R1, const float* __restrict__ W1, int D, int c, double inv,
                                               double bmm) {
    double wr = 0;
    for (int d = 0; d < D; ++d) wr += (double)W1[c * D + d] * R1[d * 64 + c];
    const double dbe = R1[D * 64 + c];
    return {dbe, inv * (wr + bmm * dbe)};
}

// parameter gradients of layers 3, 2 and 1 from the reduced partial sums
__global__ __launch_bounds__(256) void k_sa_bwd_final(
    const double* __restrict__ out3, const double* __restrict__ sums0_g, const double* __restrict__ sums0_l,
    const float* __restrict__ bnc3, const float* __restrict__ W3, const float* __restrict__ b3,
    const double* __restrict__ out2, const double* __restrict__ sums1_l, const double* __restrict__ R1_g,
    const double* __restrict__ mom_l, const float* __restrict__ bnc1, const float* __restrict__ W1,
    const float* __restrict__ b1, int D, double P, float* __restrict__ dW3, float* __restrict__ dg3,
    float* __restrict__ dbe3, float* __restrict__ dW2, float* __restrict__ dg2, float* __restrict__ dbe2,
    float* __restrict__ dW1, float* __restrict__ dg1, float* __restrict__ dbe1) {
    int r;
    switch (sa_final_segment(blockIdx.x * 256 + threadIdx.x, r)) {
    case SA_DW3: {
        const double* gram2 = out3 + SA_N_DW3;                  // out3 = [sparse3 (256,64) | sum_p a2^T a2 (64,64) | sum_p a2 (64)]
        const double* s2 = gram2 + 64 * 64;
        const int c = r >> 6, k = r & 63;
        const double mean = bn_row(bnc3, 256, BN_MEAN)[c], inv = bn_row(bnc3, 256, BN_INVSTD)[c], sc = bn_row(bnc3, 256, BN_SCALE)[c];
        double wg = 0;
        for (int j = 0; j < 64; ++j) wg += (double)W3[c * 64 + j] * gram2[j * 64 + k];
        const double yhat_a2 = inv * (wg + ((double)b3[c] - mean) * s2[k]);       // sum_p yhat3[p,c] a2[p,k]
        dW3[r] = (float)(out3[r] - (sc / P) * (sums0_g[2 * c] * s2[k] + sums0_g[2 * c + 1] * yhat_a2));
        break;
    }
    case SA_BN3: bn_store_grads(sums0_l, r, dbe3, dg3); break;
    case SA_DW2: dW2[r] = (float)out2[r]; break;
    case SA_BN2: bn_store_grads(sums1_l, r, dbe2, dg2); break;
    case SA_L1: {
        const int c = r;
        const double* R1_l = out2 + SA_N_DW2;
        const double mean = bn_row(bnc1, 64, BN_MEAN)[c], inv = bn_row(bnc1, 64, BN_INVSTD)[c], sc = bn_row(bnc1, 64, BN_SCALE)[c];
        const double bmm = (double)b1[c] - mean;
        const L1Grads l = l1_bn_grads(R1_l, W1, D, c, inv, bmm), g = l1_bn_grads(R1_g, W1, D, c, inv, bmm);
        dbe1[c] = (float)l.dbeta;
        dg1[c] = (float)l.dgamma;
        const double* sx = mom_l;
        const double* X2 = mom_l + D;
        for (int d = 0; d < D; ++d) {
            double wx = 0;
            for (int j = 0; j < D; ++j) wx += (double)W1[c * D + j] * X2[j * D + d];
            const double yhat_x = inv * (wx + bmm * sx[d]);                           // sum_p yhat1[p,c] x[p,d]
            dW1[c * D + d] = (float)(sc * (R1_l[d * 64 + c] - (g.dbeta / P) * sx[d] - (g.dgamma / P) * yhat_x));
        }
        break;
    }
    default: break;
    }
}

}  // namespace

extern "C" int facl_sa_bwd_consts3(const double* sums0, const float* bnc3, const float* W3, const float* b3, double P,
                                   float* G3, float* h3, void* stream) {
    if (!sums0 || !bnc3 || !W3 || !b3 || !G3 || !h3) return FACL_E_NULL;
    if (P < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_sa_bwd_consts3, dim3(65), dim3(256), 0, (hipStream_t)stream, sums0, bnc3, W3, b3, P, G3, h3);
    return facl_launch_status();
}

// BN backward of a row layer: (dbeta, dgamma) sums -> the two fp32 parameter gradients (THIS rank's sums) and the (2,C)
// constants kk = (dbeta/P, dgamma/P) of the SyncBN-reduced sums that facl_rows_bwd_apply / facl_segmax_bwd_apply take.
__global__ void k_bn_bwd_consts(const double* __restrict__ sums_l, const double* __restrict__ sums_g, int C, double P,
                                float* __restrict__ dbeta, float* __restrict__ dgamma, float* __restrict__ kk) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_store_grads(sums_l, c, dbeta, dgamma);
    bn_bwd_kk(sums_g[2 * c], sums_g[2 * c + 1], P, kk[c], kk[C + c]);
}

extern "C" int facl_bn_bwd_consts(const double* sums_local, const double* sums_global, int C, double P, float* dbeta,
                                  float* dgamma, float* kk, void* stream) {
    if (!sums_local || !sums_global || !dbeta || !dgamma || !kk) return FACL_E_NULL;
    if (C < 1 || P < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_bn_bwd_consts, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums_local, sums_global,
                       C, P, dbeta, dgamma, kk);
    return facl_launch_status();
}

extern "C" int facl_sa_bwd_consts2(const double* sums1, const float* bnc2, double P, float* bw2, void* stream) {
    if (!sums1 || !bnc2 || !bw2) return FACL_E_NULL;
    if (P < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_sa_bwd_consts2, dim3(1), dim3(64), 0, (hipStream_t)stream, sums1, bnc2, P, bw2);
    return facl_launch_status();
}

extern "C" int facl_sa_bwd_final(const double* out3, const double* sums0_g, const double* sums0_l, const float* bnc3,
                                 const float* W3, const float* b3, const double* out2, const double* sums1_l,
                                 const double* R1_g, const double* mom_l, const float* bnc1, const float* W1,
                                 const float* b1, int D, double P, float* dW3, float* dg3, float* dbe3, float* dW2,
                                 float* dg2, float* dbe2, float* dW1, float* dg1, float* dbe1, void* stream) {
    if (!out3 || !sums0_g || !sums0_l || !bnc3 || !W3 || !b3 || !out2 || !sums1_l || !R1_g || !mom_l || !bnc1 || !W1 ||
        !b1 || !dW3 || !dg3 || !dbe3 || !dW2 || !dg2 || !dbe2 || !dW1 || !dg1 || !dbe1)
        return FACL_E_NULL;
    if (D < FACL_SA_D_MIN || D > FACL_SA_D_MAX || P < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_sa_bwd_final, dim3((SA_FINAL_TOTAL + 255) / 256), dim3(256), 0, (hipStream_t)stream, out3, sums0_g,
                       sums0_l, bnc3, W3, b3, out2, sums1_l, R1_g, mom_l, bnc1, W1, b1, D, P, dW3, dg3, dbe3, dW2, dg2,
                       dbe2, dW1, dg1, dbe1);
    return facl_launch_status();
}

// ================================================================================================
// Frozen (eval-mode) BatchNorm: z = s y + t with s = gamma / sqrt(running_var + eps), t = beta - running_mean s, both constants.
// With dz the gradient behind the ReLU (or the max-pool routing), the same (C,2) sums the train-mode passes form -- sum dz and
// sum dz (y - mean) invstd, taken with the RUNNING mean / invstd of the (5,C) constants -- ARE dbeta and dgamma, dy = s dz has no
// batch-statistic term (kk = 0), and the bias of the conv / Linear in front gets a real gradient sum dy = s dbeta.  Nothing is
// global any more: no sum here is all-reduced.  Same style as the train-mode forms above: fp64, one thread per output, fixed order.
namespace {

__global__ void k_bn_bwd_consts_frozen(const double* __restrict__ sums, const float* __restrict__ bnc, int C,
                                       float* __restrict__ dbeta, float* __restrict__ dgamma, float* __restrict__ dbias,
                                       float* __restrict__ kk) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_store_grads(sums, c, dbeta, dgamma);
    dbias[c] = (float)((double)bn_row(bnc, C, BN_SCALE)[c] * sums[2 * c]);
    kk[c] = 0.f;
    kk[C + c] = 0.f;
}

// G3 = 0, h3 = 0: the dense part of da2 (the batch-statistic terms of BN3's backward) is gone, the sparse rows remain
__global__ void k_sa_bwd_consts3_frozen(float* __restrict__ G3, float* __restrict__ h3) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < 4096) G3[o] = 0.f;
    else if (o < 4096 + 64) h3[o - 4096] = 0.f;
}

// bw2 (4,64): dy2 = scale2*dz2 + A + B*(y2 - mean2) with A = B = 0
__global__ void k_sa_bwd_consts2_frozen(const float* __restrict__ bnc2, float* __restrict__ bw2) {
    const int c = threadIdx.x;
    if (c >= 64) return;
    bw2[c] = bn_row(bnc2, 64, BN_SCALE)[c];
    bw2[64 + c] = 0.f;
    bw2[128 + c] = 0.f;
    bw2[192 + c] = bn_row(bnc2, 64, BN_MEAN)[c];
}

// the twelve gradients of net3DV_1 (b1, b2, b3 among them) from the partial sums of the heavy passes: no Gram / sum a2 /
// x-moment term is left (out3: only its sparse part is read)
__global__ __launch_bounds__(256) void k_sa_bwd_final_frozen(
    const double* __restrict__ out3, const double* __restrict__ sums0, const float* __restrict__ bnc3,
    const double* __restrict__ out2, const double* __restrict__ sums1, const float* __restrict__ bnc2,
    const float* __restrict__ bnc1, const float* __restrict__ W1, const float* __restrict__ b1, int D,
    float* __restrict__ dW3, float* __restrict__ dg3, float* __restrict__ dbe3, float* __restrict__ db3,
    float* __restrict__ dW2, float* __restrict__ dg2, float* __restrict__ dbe2, float* __restrict__ db2,
    float* __restrict__ dW1, float* __restrict__ dg1, float* __restrict__ dbe1, float* __restrict__ db1) {
    int r;
    switch (sa_final_segment(blockIdx.x * 256 + threadIdx.x, r)) {
    case SA_DW3: dW3[r] = (float)out3[r]; break;                // sum_g coef a2[arg]: coef = scale3 dz3 is dy3 at its one position
    case SA_BN3:
        bn_store_grads(sums0, r, dbe3, dg3);
        db3[r] = (float)((double)bn_row(bnc3, 256, BN_SCALE)[r] * sums0[2 * r]);
        break;
    case SA_DW2: dW2[r] = (float)out2[r]; break;
    case SA_BN2:
        bn_store_grads(sums1, r, dbe2, dg2);
        db2[r] = (float)((double)bn_row(bnc2, 64, BN_SCALE)[r] * sums1[2 * r]);
        break;
    case SA_L1: {
        const int c = r;
        const double* R1 = out2 + SA_N_DW2;
        const double mean = bn_row(bnc1, 64, BN_MEAN)[c], inv = bn_row(bnc1, 64, BN_INVSTD)[c], sc = bn_row(bnc1, 64, BN_SCALE)[c];
        const L1Grads l = l1_bn_grads(R1, W1, D, c, inv, (double)b1[c] - mean);
        dbe1[c] = (float)l.dbeta;
        dg1[c] = (float)l.dgamma;
        db1[c] = (float)(sc * l.dbeta);
        for (int d = 0; d < D; ++d) dW1[c * D + d] = (float)(sc * R1[d * 64 + c]);
        break;
    }
    default: break;
    }
}

}  // namespace

extern "C" int facl_bn_bwd_consts_frozen(const double* sums, const float* bnc, int C, float* dbeta, float* dgamma,
                                         float* dbias, float* kk, void* stream) {
    if (!sums || !bnc || !dbeta || !dgamma || !dbias || !kk) return FACL_E_NULL;
    if (C < 1) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_bn_bwd_consts_frozen, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums, bnc, C,
                       dbeta, dgamma, dbias, kk);
    return facl_launch_status();
}

extern "C" int facl_sa_bwd_consts3_frozen(float* G3, float* h3, void* stream) {
    if (!G3 || !h3) return FACL_E_NULL;
    hipLaunchKernelGGL(k_sa_bwd_consts3_frozen, dim3((4096 + 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, G3, h3);
    return facl_launch_status();
}

extern "C" int facl_sa_bwd_consts2_frozen(const float* bnc2, float* bw2, void* stream) {
    if (!bnc2 || !bw2) return FACL_E_NULL;
    hipLaunchKernelGGL(k_sa_bwd_consts2_frozen, dim3(1), dim3(64), 0, (hipStream_t)stream, bnc2, bw2);
    return facl_launch_status();
}

extern "C" int facl_sa_bwd_final_frozen(const double* out3, const double* sums0, const float* bnc3, const double* out2,
                                        const double* sums1, const float* bnc2, const float* bnc1, const float* W1,
                                        const float* b1, int D, float* dW3, float* dg3, float* dbe3, float* db3, float* dW2,
                                        float* dg2, float* dbe2, float* db2, float* dW1, float* dg1, float* dbe1, float* db1,
                                        void* stream) {
    if (!out3 || !sums0 || !bnc3 || !out2 || !sums1 || !bnc2 || !bnc1 || !W1 || !b1 || !dW3 || !dg3 || !dbe3 || !db3 ||
        !dW2 || !dg2 || !dbe2 || !db2 || !dW1 || !dg1 || !dbe1 || !db1)
        return FACL_E_NULL;
    if (D < FACL_SA_D_MIN || D > FACL_SA_D_MAX) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_sa_bwd_final_frozen, dim3((SA_FINAL_TOTAL + 255) / 256), dim3(256), 0, (hipStream_t)stream, out3, sums0, bnc3,
                       out2, sums1, bnc2, bnc1, W1, b1, D, dW3, dg3, dbe3, db3, dW2, dg2, dbe2, db2, dW1, dg1, dbe1, db1);
    return facl_launch_status();
}
