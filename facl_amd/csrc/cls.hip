// Classifier head of supervised fine-tuning: the probe head's F.normalize on the model's own stacked, view-major
// output, and the softmax cross-entropy of the logits.  The Linear layer between them is the existing exact-split GEMM.
//
//   k_cls_gather_norm_fwd   one workgroup per clip b: reads the G + 1 rows g * B + b (g = G: the clip's global feature) straight
//                           from `stacked` with 16-byte loads, sums their squares in fp64, writes the clip-major normalised
//                           vector [x_view0 .. x_view(G-1), x_global] * inv and inv = 1 / max(||x||, 1e-12).  No permute / cat copy.
//   k_cls_gather_norm_bwd   one workgroup per clip: <dout_b, out_b> in fp64, then every one of the clip's G + 1 rows of dstacked.
//   k_softmax_ce_rows       one wave per row, lanes striding over the classes: row maximum and argmax (lowest class on equal
//                           logits), sum of exp(x - max) in fp64, dlogits = (softmax - onehot) / R, and the row's loss and its
//                           hit / bad-label flags into the workspace.
//   k_softmax_ce_finish     ONE wave: the R row losses and flags summed in a fixed order (lane l takes rows l, l + 64, ...; then
//                           the xor tree) in fp64 -> the mean and the two counters.
// Every reduction has a fixed order and no atomic takes part: the same bits every run, whatever the scheduling.
#include "common.h"
#include "norm_rows.h"
#include <limits.h>

extern "C" int64_t facl_ws_bytes(void);

namespace {

constexpr int CLS_THREADS = 256;
constexpr int CLS_WAVES = CLS_THREADS / 64;

// fp64 sum over the workgroup in a fixed order (xor tree inside a wave, then the waves 0, 1, 2, 3); all threads call.
__device__ __forceinline__ double cls_block_sum(double v, double* red) {
    v = wave_sum_f64(v);
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < CLS_WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(CLS_THREADS) void k_cls_gather_norm_fwd(const float* __restrict__ stacked, int G, int B, int C,
                                                                     float* __restrict__ out, float* __restrict__ inv_norm) {
    __shared__ double red[CLS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C4 = C >> 2, n4 = (G + 1) * C4;
    double ss = 0.0;
    for (int i = tid; i < n4; i += CLS_THREADS) {
        const int g = i / C4, c4 = i - g * C4;
        const float4 v = reinterpret_cast<const float4*>(stacked + ((size_t)g * B + b) * C)[c4];
        nr_acc_sq(ss, v);
    }
    ss = cls_block_sum(ss, red);
    const float inv = (float)nr_inv_norm(ss);                                         // F.normalize: x / max(||x||, eps)
    float4* o = reinterpret_cast<float4*>(out + (size_t)b * n4 * 4);
    for (int i = tid; i < n4; i += CLS_THREADS) {
        const int g = i / C4, c4 = i - g * C4;
        o[i] = nr_scale_f32(reinterpret_cast<const float4*>(stacked + ((size_t)g * B + b) * C)[c4], inv);
    }
    if (tid == 0) inv_norm[b] = inv;
}

__global__ __launch_bounds__(CLS_THREADS) void k_cls_gather_norm_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                                     const float* __restrict__ inv_norm, int G, int B, int C,
                                                                     float* __restrict__ dstacked) {
    __shared__ double red[CLS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C4 = C >> 2, n4 = (G + 1) * C4;
    const float4* d4 = reinterpret_cast<const float4*>(dout + (size_t)b * n4 * 4);
    const float4* o4 = reinterpret_cast<const float4*>(out + (size_t)b * n4 * 4);
    double dot = 0.0;
    for (int i = tid; i < n4; i += CLS_THREADS) {
        nr_acc_dot(dot, d4[i], o4[i]);
    }
    dot = cls_block_sum(dot, red);
    const double inv = (double)inv_norm[b];
    for (int i = tid; i < n4; i += CLS_THREADS) {
        const int g = i / C4, c4 = i - g * C4;
        reinterpret_cast<float4*>(dstacked + ((size_t)g * B + b) * C)[c4] = nr_project(inv, d4[i], o4[i], dot);
    }
}

// flags of a row: bit 0 = argmax equals the label, bit 1 = label outside [0, ncls)
__global__ __launch_bounds__(CLS_THREADS) void k_softmax_ce_rows(const float* __restrict__ logits, int ld, const int* __restrict__ labels,
                                                                 int R, int ncls, float* __restrict__ dlogits,
                                                                 double* __restrict__ row_loss, int* __restrict__ row_flags) {
    const int row = blockIdx.x * CLS_WAVES + (int)(threadIdx.x >> 6), lane = lane_id();
    if (row >= R) return;                                                            // wave-uniform
    const float* x = logits + (size_t)row * ld;
    const int lab = labels[row];
    const bool valid = lab >= 0 && lab < ncls;
    float m = -INFINITY;
    int am = INT_MAX;
    for (int c = lane; c < ncls; c += 64) {                                           // ascending: the first maximum of a lane is its lowest class
        const float v = x[c];
        if (v > m) { m = v; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    double s = 0.0;
    for (int c = lane; c < ncls; c += 64) s += exp((double)x[c] - (double)m);
    s = wave_sum_f64(s);
    if (dlogits) {
        float* d = dlogits + (size_t)row * ncls;
        const double rinv = 1.0 / (double)R;
        for (int c = lane; c < ncls; c += 64) {
            const double p = exp((double)x[c] - (double)m) / s;
            d[c] = valid ? (float)((p - (c == lab ? 1.0 : 0.0)) * rinv) : 0.f;
        }
    }
    if (lane == 0) {
        row_loss[row] = valid ? log(s) - ((double)x[lab] - (double)m) : 0.0;
        row_flags[row] = valid ? (am == lab ? 1 : 0) : 2;
    }
}

__global__ __launch_bounds__(64) void k_softmax_ce_finish(const double* __restrict__ row_loss, const int* __restrict__ row_flags, int R,
                                                          float* __restrict__ loss, int* __restrict__ stats) {
    const int lane = lane_id();
    double s = 0.0;
    int hit = 0, bad = 0;
    for (int r = lane; r < R; r += 64) {
        s += row_loss[r];
        const int f = row_flags[r];
        hit += f & 1;
        bad += (f >> 1) & 1;
    }
    s = wave_sum_f64(s);
    hit = wave_sum_i32(hit);
    bad = wave_sum_i32(bad);
    if (lane == 0) {
        loss[0] = (float)(s / (double)R);
        stats[0] = hit;
        stats[1] = bad;
    }
}

inline bool cls_shape_ok(int G, int B, int C) { return C >= 64 && C <= 1024 && C % 64 == 0 && G >= 1 && G <= 64 && B >= 1; }

}  // namespace

extern "C" int facl_cls_gather_norm_fwd(const float* stacked, int G, int B, int C, float* out, float* inv_norm, void* stream) {
    if (!cls_shape_ok(G, B, C)) return FACL_E_SHAPE;
    if (!stacked || !out || !inv_norm) return FACL_E_NULL;
    if (((uintptr_t)stacked | (uintptr_t)out) & 15) return FACL_E_ALIGN;
    k_cls_gather_norm_fwd<<<B, CLS_THREADS, 0, (hipStream_t)stream>>>(stacked, G, B, C, out, inv_norm);
    return facl_launch_status();
}

extern "C" int facl_cls_gather_norm_bwd(const float* dout, const float* out, const float* inv_norm, int G, int B, int C,
                                        float* dstacked, void* stream) {
    if (!cls_shape_ok(G, B, C)) return FACL_E_SHAPE;
    if (!dout || !out || !inv_norm || !dstacked) return FACL_E_NULL;
    if (((uintptr_t)dout | (uintptr_t)out | (uintptr_t)dstacked) & 15) return FACL_E_ALIGN;
    k_cls_gather_norm_bwd<<<B, CLS_THREADS, 0, (hipStream_t)stream>>>(dout, out, inv_norm, G, B, C, dstacked);
    return facl_launch_status();
}

extern "C" int facl_softmax_ce(const float* logits, int ld, const int* labels, int R, int ncls, float* loss, float* dlogits,
                               int* stats, void* ws, void* stream) {
    if (ncls < 2 || ncls > 1024 || R < 1 || ld < ncls) return FACL_E_SHAPE;
    if ((size_t)R * (sizeof(double) + sizeof(int)) > (size_t)facl_ws_bytes()) return FACL_E_SHAPE;
    if (!logits || !labels || !loss || !stats || !ws) return FACL_E_NULL;
    if ((uintptr_t)ws & 7) return FACL_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* row_loss = reinterpret_cast<double*>(ws);
    int* row_flags = reinterpret_cast<int*>(row_loss + R);
    k_softmax_ce_rows<<<(R + CLS_WAVES - 1) / CLS_WAVES, CLS_THREADS, 0, st>>>(logits, ld, labels, R, ncls, dlogits, row_loss, row_flags);
    k_softmax_ce_finish<<<1, 64, 0, st>>>(row_loss, row_flags, R, loss, stats);
    return facl_launch_status();
}
