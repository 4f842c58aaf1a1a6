// Prediction with a trained head: class probabilities of the logits accumulated over test-time draws, and the k
// most probable classes of every row with the rank of its label.
//
//   k_cls_probs_acc   one wave per row, lanes striding over the classes: the row maximum (and whether any logit is NaN), the
//                     sum of exp(x - max) in fp64 (lane partial sums, then the xor tree), acc = [acc +] exp(x - max) / sum in
//                     fp64.  A row whose maximum is not finite is stored as NaN.
//   k_cls_topk        one wave per row, lane l holds the classes l, l + 64, .. (<= 16 of them) in registers: k rounds of a wave
//                     argmax under (value descending, class ascending); the winner of round e stays in lane e, which writes
//                     list entry e.  The label's rank is a count over all classes, summed over the wave.
// Every reduction has a fixed order and no atomic takes part: the same bits every run, whatever the scheduling.
#include "common.h"
#include <limits.h>

namespace {

constexpr int PRED_THREADS = 256;
constexpr int PRED_WAVES = PRED_THREADS / 64;
constexpr int PRED_MAX_CLS = 1024;
constexpr int PRED_PER_LANE = PRED_MAX_CLS / 64;

__global__ __launch_bounds__(PRED_THREADS) void k_cls_probs_acc(const float* __restrict__ logits, int ld, int R, int ncls,
                                                                double* __restrict__ acc, int first) {
    const int row = blockIdx.x * PRED_WAVES + (int)(threadIdx.x >> 6), lane = lane_id();
    if (row >= R) return;                                                            // wave-uniform
    const float* x = logits + (size_t)row * ld;
    double* a = acc + (size_t)row * ncls;
    float m = -INFINITY;
    bool nan = false;
    for (int c = lane; c < ncls; c += 64) {
        const float v = x[c];
        nan |= v != v;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        m = om > m ? om : m;
    }
    if (__any(nan) || m == INFINITY || m == -INFINITY) {                             // wave-uniform: NaN, +inf, or nothing but -inf
        for (int c = lane; c < ncls; c += 64) a[c] = __builtin_nan("");
        return;
    }
    double s = 0.0;
    for (int c = lane; c < ncls; c += 64) s += exp((double)x[c] - (double)m);
    s = wave_sum_f64(s);
    for (int c = lane; c < ncls; c += 64) {
        const double p = exp((double)x[c] - (double)m) / s;
        a[c] = first ? p : a[c] + p;
    }
}

// (v, c) precedes (bv, bc) in the order (value descending, class ascending); an empty slot is (-inf, INT_MAX)
__device__ __forceinline__ bool pred_precedes(double v, int c, double bv, int bc) { return v > bv || (v == bv && c < bc); }

__global__ __launch_bounds__(PRED_THREADS) void k_cls_topk(const double* __restrict__ acc, int R, int ncls, double ndraws, int k,
                                                           const int* __restrict__ labels, float* __restrict__ top_p,
                                                           int* __restrict__ top_c, int* __restrict__ rank) {
    const int row = blockIdx.x * PRED_WAVES + (int)(threadIdx.x >> 6), lane = lane_id();
    if (row >= R) return;                                                            // wave-uniform
    const double* a = acc + (size_t)row * ncls;
    double v[PRED_PER_LANE];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < PRED_PER_LANE; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < ncls ? a[c] : 0.0;
        nan |= v[j] != v[j];
    }
    if (__any(nan)) {                                                                // wave-uniform
        if (lane < k) {
            top_p[(size_t)row * k + lane] = __builtin_nanf("");
            top_c[(size_t)row * k + lane] = -1;
        }
        if (labels && lane == 0) rank[row] = -1;
        return;
    }
    if (labels) {
        const int lab = labels[row];
        if (lab < 0 || lab >= ncls) {
            if (lane == 0) rank[row] = -2;
        } else {
            const double lv = a[lab];
            int n = 0;
#pragma unroll
            for (int j = 0; j < PRED_PER_LANE; ++j) {
                const int c = lane + 64 * j;
                n += (c < ncls && pred_precedes(v[j], c, lv, lab)) ? 1 : 0;
            }
            n = wave_sum_i32(n);
            if (lane == 0) rank[row] = n;
        }
    }
    unsigned taken = 0;                                                               // bit j: class lane + 64 j is in the list
    double my_v = 0.0;
    int my_c = -1;
    for (int e = 0; e < k; ++e) {
        double bv = -INFINITY;
        int bc = INT_MAX;
#pragma unroll
        for (int j = 0; j < PRED_PER_LANE; ++j) {
            const int c = lane + 64 * j;
            if (c < ncls && !((taken >> j) & 1u) && pred_precedes(v[j], c, bv, bc)) { bv = v[j]; bc = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (pred_precedes(ov, oc, bv, bc)) { bv = ov; bc = oc; }
        }
        // k <= ncls: a class is left in every round, so bc is one of them, the same in all lanes
        if ((bc & 63) == lane) taken |= 1u << (bc >> 6);
        if (lane == e) { my_v = bv; my_c = bc; }
    }
    if (lane < k) {
        top_p[(size_t)row * k + lane] = (float)(my_v / ndraws);
        top_c[(size_t)row * k + lane] = my_c;
    }
}

inline bool pred_shape_ok(int R, int ncls) { return ncls >= 2 && ncls <= PRED_MAX_CLS && R >= 1; }

}  // namespace

extern "C" int facl_cls_probs_acc(const float* logits, int ld, int R, int ncls, double* acc, int first, void* stream) {
    if (!pred_shape_ok(R, ncls) || ld < ncls) return FACL_E_SHAPE;
    if (!logits || !acc) return FACL_E_NULL;
    if ((uintptr_t)acc & 7) return FACL_E_ALIGN;
    k_cls_probs_acc<<<(R + PRED_WAVES - 1) / PRED_WAVES, PRED_THREADS, 0, (hipStream_t)stream>>>(logits, ld, R, ncls, acc, first);
    return facl_launch_status();
}

extern "C" int facl_cls_topk(const double* acc, int R, int ncls, int ndraws, int k, const int32_t* labels, float* top_p,
                             int32_t* top_c, int32_t* rank, void* stream) {
    if (!pred_shape_ok(R, ncls) || ndraws < 1 || k < 1 || k > 64 || k > ncls) return FACL_E_SHAPE;
    if (!acc || !top_p || !top_c || (labels && !rank)) return FACL_E_NULL;
    if ((uintptr_t)acc & 7) return FACL_E_ALIGN;
    k_cls_topk<<<(R + PRED_WAVES - 1) / PRED_WAVES, PRED_THREADS, 0, (hipStream_t)stream>>>(acc, R, ncls, (double)ndraws, k, labels,
                                                                                            top_p, top_c, rank);
    return facl_launch_status();
}
