// The BatchNorm constants and the fp64 arithmetic that makes them, written ONCE (finalize.hip, fchead.hip; rows_common.h takes
// the row names): the (5, C) layout, statistics -> constants -> running buffers, the activation bound, the backward constants,
// the BN1 moment sums and the folded layer-1 table.  The library is built with -ffp-contract=off, so an expression written here
// gives the same bits in every kernel it is inlined into: k_sa_bn1_chain equals its three launches, and k_fc_finalize equals two
// facl_bn_finalize calls, by construction.
// BN semantics: cn3d_model_conbag.py:46,50,54,64,68,72,84 (nn.BatchNorm2d/1d defaults: eps 1e-5, momentum 0.1, biased variance to
// normalise, unbiased for the running buffer).
#pragma once
#include "common.h"

// ---- the constants "bnc" (5, C), or (2, 5, C) for the two row segments of the FC head ------------------------------------------
enum BnRow { BN_MEAN, BN_INVSTD, BN_SCALE, BN_SHIFT, BN_SIGN, BN_ROWS };
// the (5, C) block of segment seg; row r of segment seg
template <class T>
__device__ __forceinline__ T* bn_segment(T* bnc, int C, int seg) { return bnc + (size_t)seg * BN_ROWS * C; }
template <class T>
__device__ __forceinline__ T* bn_row(T* bnc, int C, int r, int seg = 0) { return bn_segment(bnc, C, seg) + r * C; }

// ---- train mode: (sum, sumsq) over `count` values -> mean, biased variance clamped at 0, invstd --------------------------------
struct BnStats { double mean, var, invstd; };
__device__ __forceinline__ BnStats bn_train_stats(double sum, double sumsq, double count, float eps) {
    const double mean = sum / count;
    double var = sumsq / count - mean * mean;
    if (var < 0) var = 0;
    return {mean, var, 1.0 / sqrt(var + (double)eps)};
}

// column c of the five rows.  `mean32` is stored as it is (eval mode: the running mean itself, not a rounded copy of a copy); `g`
// makes scale and shift (eval mode poisons it), the sign row always comes from the real `gamma`.  Returns (scale, shift) as stored.
struct BnAffine { float scale, shift; };
__device__ __forceinline__ BnAffine bn_store_consts(float* __restrict__ bnc, int C, int c, float mean32, double mean, double invstd,
                                                    double g, double b, float gamma) {
    const BnAffine a = {(float)(g * invstd), (float)(b - mean * g * invstd)};
    bn_row(bnc, C, BN_MEAN)[c] = mean32;
    bn_row(bnc, C, BN_INVSTD)[c] = (float)invstd;
    bn_row(bnc, C, BN_SCALE)[c] = a.scale;
    bn_row(bnc, C, BN_SHIFT)[c] = a.shift;
    bn_row(bnc, C, BN_SIGN)[c] = gamma < 0 ? -1.0f : 1.0f;
    return a;
}

// one update of the running buffers (unbiased variance), rounded to fp32 at its end: two updates in a row round in between
__device__ __forceinline__ void bn_running_step(float& rm, float& rv, float momentum, double mean, double var, double count) {
    const double unb = count > 1 ? var * count / (count - 1) : var;
    rm = (float)((1.0 - momentum) * rm + momentum * mean);
    rv = (float)((1.0 - momentum) * rv + momentum * unb);
}

// BOUND of max|gamma (y - mean) invstd + beta| over the batch the statistics were taken on: Samuelson's inequality,
// |y_i - mean| <= sigma sqrt(n - 1) for ANY n numbers, gives |.| <= |gamma| sqrt(n - 1) sigma invstd + |beta| (sigma invstd =
// sqrt(var / (var + eps)) <= 1).  It is the fp16x3 scale of the layer's activation (common.h) -- rigorous, no pass over the data,
// and within a few octaves of the true maximum.  1.001: fp32 rounding of the constants.
__device__ __forceinline__ float bn_act_bound(double g, double b, double var, double invstd, double count) {
    return (float)((fabs(g) * sqrt((count > 1 ? count - 1 : 1) * var) * invstd + fabs(b)) * 1.001);
}

__device__ __forceinline__ float bn_wave_max(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}
// the maximum of `bound` over the workgroup, STORED into every one of the FACL_AMAX_SLOTS slots of `amax`.  All threads call;
// ONE_WAVE: a 64-thread launch (else the waves meet in LDS: one barrier, at most 16 waves = 1024 threads).  fmaxf drops a NaN bound.
template <bool ONE_WAVE>
__device__ __forceinline__ void bn_store_bound_in_slots(float bound, unsigned* __restrict__ amax) {
    bound = bn_wave_max(bound);
    if constexpr (!ONE_WAVE) {
        __shared__ float red[16];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bound;
        __syncthreads();
        bound = red[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) bound = fmaxf(bound, red[w]);
    }
    if (threadIdx.x < FACL_AMAX_SLOTS) amax[threadIdx.x * FACL_AMAX_STRIDE] = __float_as_uint(bound);
}

// ---- backward: the (dbeta, dgamma) sums of channel c are the parameter gradients; kk = (dbeta / P, dgamma / P) of the
// (all-reduced) sums, in the arithmetic of the torch glue it replaces: fp32 sum times fp32 reciprocal count
__device__ __forceinline__ void bn_store_grads(const double* __restrict__ sums, int c, float* __restrict__ dbeta, float* __restrict__ dgamma) {
    dbeta[c] = (float)sums[2 * c];
    dgamma[c] = (float)sums[2 * c + 1];
}
__device__ __forceinline__ void bn_bwd_kk(double dbeta_sum, double dgamma_sum, double P, float& k1, float& k2) {
    const float inv = (float)(1.0 / P);
    k1 = (float)dbeta_sum * inv;
    k2 = (float)dgamma_sum * inv;
}

// ---- layer 1 of the SA point-MLP -----------------------------------------------------------------------------------------------
// BN1 statistics of channel c analytically from the input moments mom = [sx (D) | X2 (D,D)]: y1 = W1 x + b1  =>
//   sum_p y1_c = W1_c . sx + P b1_c ;  sum_p y1_c^2 = W1_c X2 W1_c^T + 2 b1_c W1_c . sx + P b1_c^2
__device__ __forceinline__ void bn1_moment_sums(const double* __restrict__ mom, double count, int D, const float* __restrict__ W1,
                                                const float* __restrict__ b1, int c, double& su, double& sq) {
    const double* sx = mom;
    const double* X2 = mom + D;
    double ws = 0, q = 0;
    for (int i = 0; i < D; ++i) {
        const double wi = W1[c * D + i];
        ws += wi * sx[i];
        double t = 0;
        for (int j = 0; j < D; ++j) t += X2[i * D + j] * (double)W1[c * D + j];
        q += wi * t;
    }
    const double b = b1[c];
    su = ws + count * b;
    sq = q + 2.0 * b * ws + count * b * b;
}

// row c of the table that folds BN1 into the first 1x1 conv: a1 = relu((scale*W1) x + (scale*b1 + shift)); FACL_SA_L1_COLS(D)
// floats (8, or 12 for D > 4: include/facl_hip.h).  Returns the L1 norm of the folded weights and the folded bias.
struct L1Row { float l1, bias; };
__device__ __forceinline__ L1Row l1tab_row(const float* __restrict__ W1, const float* __restrict__ b1, int D, int c, float scale,
                                           float shift, float* __restrict__ tab) {
    const int L = FACL_SA_L1_COLS(D);
    L1Row r = {0.f, scale * b1[c] + shift};
    for (int i = 0; i < L - 4; ++i) {
        const float w = i < D ? scale * W1[c * D + i] : 0.0f;
        tab[c * L + i] = w;
        r.l1 += fabsf(w);
    }
    tab[c * L + L - 4] = r.bias;
    tab[c * L + L - 3] = tab[c * L + L - 2] = tab[c * L + L - 1] = 0.0f;
    return r;
}
