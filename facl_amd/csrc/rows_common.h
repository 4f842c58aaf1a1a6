// Shared pieces of the encoder tail's row kernels (rows.hip, fchead.hip; the dgrad epilogue of gemm_rs.hip takes the element
// helpers): the BatchNorm + ReLU arithmetic per element, per-lane-component application of it, the 4-phase block reduction,
// the max-pool compare and the max|dy| bookkeeping.  The library is built with -ffp-contract=off and the one fused operation is
// an explicit fmaf, so an expression written here gives the same bits in every kernel it is inlined into.
#pragma once
#include "bn_consts.h"

// all pointers 16-byte aligned (the float4 forms need it)
template <class... P>
static inline bool aligned16(const P*... p) { return !((... | (uintptr_t)p) & 15); }

// ---- BatchNorm + ReLU, forward and backward, per element -------------------------------------------------------------------
// consts "bnc" (5,C) = mean, invstd, scale, shift, sgn (bn_consts.h: BnRow);  kk (2,C): k1 = dbeta/P, k2 = dgamma/P
__device__ __forceinline__ float bn_relu(float scale, float y, float shift) { return relu_nan(fmaf(scale, y, shift)); }
// dz = dout * [z > 0]: the edge z == 0 and a NaN z both close the gate
__device__ __forceinline__ float bn_relu_dz(float scale, float y, float shift, float dout) { return fmaf(scale, y, shift) > 0.f ? dout : 0.f; }
__device__ __forceinline__ float bn_yhat(float y, float mean, float inv) { return (y - mean) * inv; }
__device__ __forceinline__ float bn_bwd_dy(float scale, float dz, float k1, float yhat, float k2) { return scale * (dz - k1 - yhat * k2); }
// dy of relu(bn(y)) from dout
__device__ __forceinline__ float bn_relu_bwd(float dout, float y, float mean, float inv, float scale, float shift, float k1, float k2) {
    return bn_bwd_dy(scale, bn_relu_dz(scale, y, shift, dout), k1, bn_yhat(y, mean, inv), k2);
}

// ---- a lane's W channels: W = 4 (float4 / int4, C % 4 == 0 and 16-byte aligned tensors) or W = 1 (the fallback) -------------
template <int W> struct lanes { using F = float4; using I = int4; };
template <> struct lanes<1> { using F = float; using I = int; };
// component E of a quad; a scalar stands for four equal components
template <int E> __device__ __forceinline__ float quad_at(const float4& v) { return E == 0 ? v.x : E == 1 ? v.y : E == 2 ? v.z : v.w; }
template <int E> __device__ __forceinline__ int quad_at(const int4& v) { return E == 0 ? v.x : E == 1 ? v.y : E == 2 ? v.z : v.w; }
template <int E> __device__ __forceinline__ float quad_at(float v) { return v; }
template <int E> __device__ __forceinline__ int quad_at(int v) { return v; }
// f(e, a[e]...) for each of the lane's W components e
template <int W, class Fn, class... A>
__device__ __forceinline__ void lane_each(Fn f, const A&... a) {
    if constexpr (W == 1) f(0, a...);
    else { f(0, quad_at<0>(a)...); f(1, quad_at<1>(a)...); f(2, quad_at<2>(a)...); f(3, quad_at<3>(a)...); }
}
// the lane's W results f(a[e]...)
template <int W, class Fn, class... A>
__device__ __forceinline__ typename lanes<W>::F lane_map(Fn f, const A&... a) {
    if constexpr (W == 1) return f(a...);
    else return make_float4(f(quad_at<0>(a)...), f(quad_at<1>(a)...), f(quad_at<2>(a)...), f(quad_at<3>(a)...));
}

// the lane's columns cw of the (5,C) constants (C = W * CW) and of kk
template <int W> struct BnLanes { typename lanes<W>::F mean, inv, scale, shift; };
template <int W>
__device__ __forceinline__ BnLanes<W> bn_lanes(const float* bnc, int C, int cw) {
    using F = typename lanes<W>::F;
    return {reinterpret_cast<const F*>(bn_row(bnc, C, BN_MEAN))[cw], reinterpret_cast<const F*>(bn_row(bnc, C, BN_INVSTD))[cw],
            reinterpret_cast<const F*>(bn_row(bnc, C, BN_SCALE))[cw], reinterpret_cast<const F*>(bn_row(bnc, C, BN_SHIFT))[cw]};
}
template <int W> struct KkLanes { typename lanes<W>::F k1, k2; };
template <int W>
__device__ __forceinline__ KkLanes<W> kk_lanes(const float* kk, int C, int cw) {
    using F = typename lanes<W>::F;
    return {reinterpret_cast<const F*>(kk)[cw], reinterpret_cast<const F*>(kk + C)[cw]};
}

// backward statistics of relu(bn(y)) over the rows r0, r0 + step, .. < r1 of the lane's columns: acc[2e] += dz, acc[2e + 1] += dz * yhat
// (exact fp32 x fp32 products, fp64 sums)
template <int W>
__device__ __forceinline__ void bn_bwd_stats_rows(const float* __restrict__ dout, const float* __restrict__ y, int CW, int cw,
                                                  const float* __restrict__ bnc, int r0, int r1, int step, double (&acc)[2 * W]) {
    using F = typename lanes<W>::F;
    const BnLanes<W> q = bn_lanes<W>(bnc, W * CW, cw);
    for (int r = r0; r < r1; r += step) {
        const size_t o = (size_t)r * CW + cw;
        const F v = reinterpret_cast<const F*>(y)[o];
        const F d = lane_map<W>(bn_relu_dz, q.scale, v, q.shift, reinterpret_cast<const F*>(dout)[o]);
        lane_each<W>([&](int e, float d, float v, float mean, float inv) {
            acc[2 * e] += (double)d;
            acc[2 * e + 1] += (double)d * (double)bn_yhat(v, mean, inv);
        }, d, v, q.mean, q.inv);
    }
}

// ---- block = 64 lanes x 4 phases: the phases' N partial sums per lane meet in LDS and are added in phase order ---------------
// `red` is the kernel's own __shared__ double[3][64][N].  ALL 256 threads of the block must call (one barrier inside: no early
// return in front of it); true in the phase-0 threads of `live` lanes, whose acc then holds ((p0 + p1) + p2) + p3.
template <int N>
__device__ __forceinline__ bool phase_sum(double (&acc)[N], double (&red)[3][64][N], int lane, int ph, bool live) {
    if (ph > 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) red[ph - 1][lane][e] = acc[e];
    }
    __syncthreads();
    if (ph != 0 || !live) return false;
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = ((acc[e] + red[0][lane][e]) + red[1][lane][e]) + red[2][lane][e];
    return true;
}

// ---- max-pool walk: strictly greater, or NaN, replaces -- the first maximum wins, a NaN wins and stays (MaxPool2d propagates it)
__device__ __forceinline__ void first_max_wins(float& best, int& bi, float v, int idx) {
    if (v > best || v != v) { best = v; bi = idx; }
}
template <class I>                                      // idx: one index per component (int4) or the same for all four (int)
__device__ __forceinline__ void first_max_wins(float4& best, int4& bi, const float4& v, const I& idx) {
    first_max_wins(best.x, bi.x, v.x, quad_at<0>(idx)); first_max_wins(best.y, bi.y, v.y, quad_at<1>(idx));
    first_max_wins(best.z, bi.z, v.z, quad_at<2>(idx)); first_max_wins(best.w, bi.w, v.w, quad_at<3>(idx));
}

// ---- max|.| of the tensor a kernel writes, for the consumers that scale it by a power of two (fp16x3 GEMMs, common.h) ---------
// The bit pattern of a non-negative float orders like the unsigned integer, NaN above everything (so a NaN gradient stays visible).
// The maximum lives in FACL_AMAX_SLOTS slots, one 128-byte line each (a workgroup uses slot = its linear id mod the slot
// count: thousands of atomics on ONE address serialise in the L2 -- measured, the pass doubled in time); the consumer takes
// the maximum over the slots.  A wave reads its slot when it STARTS and skips the atomic when it cannot raise that value
// (a stale read only costs a redundant atomic).  Lanes that left early (channel tail) are absent from the exchange.
__device__ __forceinline__ float abs_max4(float m, const float4& v) {
    const unsigned a = __float_as_uint(m);
    unsigned b = __float_as_uint(v.x) & 0x7fffffffu, c = __float_as_uint(v.y) & 0x7fffffffu;
    unsigned d = __float_as_uint(v.z) & 0x7fffffffu, e = __float_as_uint(v.w) & 0x7fffffffu;
    b = b > c ? b : c; d = d > e ? d : e; b = b > d ? b : d;
    return __uint_as_float(a > b ? a : b);
}
__device__ __forceinline__ unsigned* abs_max_slot(unsigned* amax) {
    return amax + (size_t)((blockIdx.x + blockIdx.y * gridDim.x) & (FACL_AMAX_SLOTS - 1)) * FACL_AMAX_STRIDE;
}
__device__ __forceinline__ void publish_abs_max(unsigned* slot, unsigned seen, float m) {
    const unsigned b = __float_as_uint(m);
    if (b > seen) atomicMax(slot, b);                                   // the compiler folds a wave's lanes into one atomic
}
