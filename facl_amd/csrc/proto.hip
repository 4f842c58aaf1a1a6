// Prototype contrastive term on the k-means centroids (ProtoNCE): loss and d(loss)/d(stacked) in ONE pass over the rows.
//
//   z_r = x_r / max(||x_r||, 1e-12),  p_k = c_k proto_inv_k,  l_rk = a_k <z_r, p_k>,  s_r = classes[r % B]
//   loss = (1/M) sum over the rows with 0 <= s_r < K of [logsumexp_k l_rk - l_{r,s_r}]
//   dx_r = inv_r (dz_r - z_r <dz_r, z_r>),  dz_r = sum_k (softmax_k(l_r.) - [k = s_r]) / M * a_k p_k      (0 for the other rows)
//
//   k_proto_nce     workgroup = PN_ROWS (16) rows x 8 waves; the exact f32-input MFMA v_mfma_f32_16x16x4_f32 throughout.
//     0  wave w normalises rows 2w, 2w + 1: fp64 sum of squares through the shared row body (norm_rows.h), z rounded once, into LDS.
//     1  logits: the prototypes in tiles of 16, tile t on wave t % 8.  A lane (n = lane & 15, q = lane >> 4) reads the float4
//        z[n][16 j + 4 q ..] from LDS and the float4 c[16 t + n][16 j + 4 q ..] from global memory: element e of the two feeds
//        MFMA e of the step, i.e. the k index of a sum is permuted, which a sum does not mind.  A prototype element is used by
//        exactly one wave of the workgroup, so staging it through LDS would buy no reuse; a lane group reads 64 contiguous bytes
//        of 16 rows, and the other half of each 128-byte line on the next j.  Four accumulators per tile (chains of C / 4
//        products) are added at the end; the logit is (acc * proto_inv_k) * a_k and goes to LDS (16 x K).
//     2  wave w takes rows 2w, 2w + 1 of the logits: maximum, sum of exp in fp64, the row's loss term,
//        and the coefficients (softmax - onehot) / M * a_k proto_inv_k, rounded once, over the logits in LDS; zeros past K.
//     3  dz = coef (16 x K) . c (K x C): wave w owns columns 64 w .. 64 w + 63 (C / 64 <= 8 waves work); lane (n, q) reads the
//        float4 coef[n][16 t + 4 q ..] from LDS and, for e = 0..3, the float4 c[16 t + 4 q + e][64 w + 4 n ..] from global memory
//        (4 rows x 256 contiguous bytes per load): 16 MFMAs per 16 prototypes into four accumulators, whose register i is row
//        4 q + i and whose lane is columns 64 w + 4 n + {0..3}: the projection through the normalisation (fp64, one rounding per
//        element) and the 16-byte store of dx need no exchange but the row's <dz, z>, summed over the 16 lanes of a group
//        (xor tree), then over the waves in order.
//   k_proto_finish  ONE wave: the workgroups' loss sums in a fixed order (lane l takes l, l + 64, ...; xor tree), / M, one rounding.
// LDS images: rows of C + 4 and of 16 ceil(K / 16) + 4 floats: the row stride is 4 banks mod 64, so the 16 rows a ds_read_b128 lane
// group touches at one q start on 16 different 16-byte slots; groups that mix two q (MI355X: {0-3, 12-15, 20-27}, ...) meet on
// one slot at most twice.  Reads are 1 per 4 MFMAs (32 cycles each): the MFMA pipe, not the LDS, sets the pace.
// Determinism: no floating-point atomic; every sum runs in an order fixed by (M, C, K) alone.  The one atomic is the integer OR
// that raises `err` for a class id >= K; such a row, like a row of unknown class (< 0), gets zeros and adds nothing, and the id is
// compared BEFORE it indexes anything.  Prototype rows past K (the last tile) are clamped to row K - 1 before the address is
// formed and what they load is replaced by 0.
#include "common.h"
#include "norm_rows.h"

namespace {

constexpr int PN_ROWS = 16;                    // rows of a workgroup: one MFMA tile
constexpr int PN_WAVES = 8;
constexpr int PN_THREADS = 64 * PN_WAVES;
constexpr int PN_KMAX = 1024, PN_CMAX = 512;
constexpr int PN_PAD = 4;                      // floats: LDS row strides of 4 banks mod 64
constexpr int PN_E_CLASS = 1;
constexpr int PN_NDBL = 3 * PN_ROWS + PN_WAVES * PN_ROWS;     // inv, loss, known, <dz, z> per wave

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

inline __host__ __device__ int pn_kpad(int K) { return (K + 15) & ~15; }
inline size_t pn_lds_bytes(int C, int K) {
    return (size_t)PN_NDBL * 8 + (size_t)PN_ROWS * ((size_t)(C + PN_PAD) + (size_t)(pn_kpad(K) + PN_PAD)) * 4;
}
constexpr int PN_LDS_MAX = PN_NDBL * 8 + PN_ROWS * ((PN_CMAX + PN_PAD) + (PN_KMAX + PN_PAD)) * 4;

__global__ __launch_bounds__(PN_THREADS) void k_proto_nce(const float* __restrict__ x, int M, int ld, int C, int B,
                                                          const int* __restrict__ classes, const float* __restrict__ protos,
                                                          const float* __restrict__ proto_inv, const float* __restrict__ scale, int K,
                                                          float* __restrict__ dx, double* __restrict__ part, int* __restrict__ err) {
    extern __shared__ double pn_lds[];
    double* s_inv = pn_lds;                                                            // [16] 1 / max(||x||, eps); 0 past M
    double* s_loss = s_inv + PN_ROWS;                                                  // [16] the row's loss term
    double* s_known = s_loss + PN_ROWS;                                                // [16] 1.0: 0 <= class < K
    double* s_dot = s_known + PN_ROWS;                                            // [8][16] <dz, z> of a wave's columns
    float* zs = reinterpret_cast<float*>(pn_lds + PN_NDBL);                            // [16][C + 4]
    const int ZS = C + PN_PAD, KP = pn_kpad(K), LS = KP + PN_PAD;
    float* lg = zs + PN_ROWS * ZS;                                                     // [16][KP + 4] logits, then coefficients
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * PN_ROWS;

    // ---- 0: normalise -------------------------------------------------------------------------------------------------------------
    const int C4 = C >> 2;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = wave * 2 + rr, row = r0 + rl;
        const bool live = row < M;                                                     // wave-uniform
        float4 v[2];
        double ss = 0.0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c4 = lane + 64 * u;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && c4 < C4) v[u] = reinterpret_cast<const float4*>(x + (size_t)row * ld)[c4];
            nr_acc_sq(ss, v[u]);
        }
        ss = wave_sum_f64(ss);
        const double inv = live ? nr_inv_norm(ss) : 0.0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c4 = lane + 64 * u;
            if (c4 < C4) *reinterpret_cast<float4*>(zs + rl * ZS + 4 * c4) = nr_scale_f64(v[u], inv);
        }
        if (lane == 0) s_inv[rl] = inv;
    }
    __syncthreads();

    // ---- 1: logits ----------------------------------------------------------------------------------------------------------------
    for (int t = wave; t < KP / 16; t += PN_WAVES) {
        const int pk = 16 * t + n;
        const bool ok = pk < K;
        const int pkc = ok ? pk : K - 1;                                               // clamped before the address is formed
        const float4* bp = reinterpret_cast<const float4*>(protos + (size_t)pkc * C) + q;
        const float4* ap = reinterpret_cast<const float4*>(zs + n * ZS) + q;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < C / 16; j += 4) {                                          // C % 64 == 0: four loads of each operand in flight
            float4 a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = ap[4 * (j + u)]; b[u] = bp[4 * (j + u)]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a0 = MFMA16(a[u].x, b[u].x, a0); a1 = MFMA16(a[u].y, b[u].y, a1);
                a2 = MFMA16(a[u].z, b[u].z, a2); a3 = MFMA16(a[u].w, b[u].w, a3);
            }
        }
        const f32x4 acc = (a0 + a1) + (a2 + a3);
        const float pi = proto_inv[pkc], sc = scale[pkc];
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[(4 * q + i) * LS + pk] = ok ? acc[i] * pi * sc : 0.f;   // register i: row 4 q + i, column n
    }
    __syncthreads();

    // ---- 2: softmax statistics, loss terms, coefficients ------------------------------------------------------------------------------
    const double rinv_m = 1.0 / (double)M;
#pragma unroll 1
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = wave * 2 + rr, row = r0 + rl;
        const int cls = row < M ? classes[row % B] : -1;                               // wave-uniform
        const bool known = cls >= 0 && cls < K;
        float* L = lg + rl * LS;
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, L[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const double lown = (double)L[known ? cls : 0] - (double)m;                    // read before the row is overwritten
        double s = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {                                         // 0: the sum of exp; 1: the exp again, into the
            for (int k = lane; k < KP; k += 64) {                                      // coefficients (one site of the fp64 exp)
                const double ex = k < K ? exp((double)L[k] - (double)m) : 0.0;
                if (pass == 0) {
                    s += ex;
                } else {
                    float cf = 0.f;
                    if (known && k < K) cf = (float)((ex / s - (k == cls ? 1.0 : 0.0)) * rinv_m * ((double)scale[k] * (double)proto_inv[k]));
                    L[k] = cf;
                }
            }
            if (pass == 0) s = wave_sum_f64(s);
        }
        if (lane == 0) {
            s_loss[rl] = known ? log(s) - lown : 0.0;
            s_known[rl] = known ? 1.0 : 0.0;
            if (cls >= K) atomicOr(err, PN_E_CLASS);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < PN_ROWS; ++i) s += s_loss[i];
        part[blockIdx.x] = s;
    }

    // ---- 3: dz = coef . c, projected through the normalisation ------------------------------------------------------------------------
    const bool work = wave < C / 64;                                                   // wave-uniform
    const int colb = work ? 64 * wave + 4 * n : 0;
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0, d2 = d0, d3 = d0;
    if (work) {
        const float4* ap = reinterpret_cast<const float4*>(lg + n * LS) + q;
        for (int t = 0; t < KP / 16; ++t) {
            const float4 a = ap[4 * t];
            float4 b[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pk = 16 * t + 4 * q + e;
                const bool ok = pk < K;
                b[e] = *reinterpret_cast<const float4*>(protos + (size_t)(ok ? pk : K - 1) * C + colb);
                if (!ok) b[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d0 = MFMA16(av[e], b[e].x, d0); d1 = MFMA16(av[e], b[e].y, d1);
                d2 = MFMA16(av[e], b[e].z, d2); d3 = MFMA16(av[e], b[e].w, d3);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = 4 * q + i;
            const float4 d = make_float4(d0[i], d1[i], d2[i], d3[i]);
            const float4 z = *reinterpret_cast<const float4*>(zs + rl * ZS + colb);
            double dot = 0.0;
            nr_acc_dot(dot, d, z);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);              // the 16 lanes of a group: the row's columns of this wave
            if (n == 0) s_dot[wave * PN_ROWS + rl] = dot;
        }
    }
    __syncthreads();
    if (work) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = 4 * q + i, row = r0 + rl;
            if (row >= M) continue;
            float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s_known[rl] != 0.0) {
                double dot = 0.0;
                for (int w = 0; w < C / 64; ++w) dot += s_dot[w * PN_ROWS + rl];
                const float4 d = make_float4(d0[i], d1[i], d2[i], d3[i]);
                const float4 z = *reinterpret_cast<const float4*>(zs + rl * ZS + colb);
                out = nr_project(s_inv[rl], d, z, dot);
            }
            *reinterpret_cast<float4*>(dx + (size_t)row * C + colb) = out;
        }
    }
}

__global__ __launch_bounds__(64) void k_proto_finish(const double* __restrict__ part, int nparts, int M, float* __restrict__ loss) {
    const int lane = lane_id();
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += part[i];
    s = wave_sum_f64(s);
    if (lane == 0) loss[0] = (float)(s / (double)M);
}

inline int pn_blocks(int M) { return (M + PN_ROWS - 1) / PN_ROWS; }

}  // namespace

extern "C" int64_t facl_proto_nce_ws_bytes(int M) {
    if (M < 1) return FACL_E_SHAPE;
    return (int64_t)(((size_t)pn_blocks(M) * 8 + 255) & ~(size_t)255);
}

extern "C" int facl_proto_nce(const float* stacked, int M, int ld, int C, int B, const int32_t* classes, const float* protos,
                              const float* proto_inv, const float* scale, int K, float* loss, float* dstacked, int32_t* err, void* ws,
                              void* stream) {
    if (M < 1 || B < 1 || M % B != 0 || K < 1 || K > PN_KMAX || C < 64 || C > PN_CMAX || C % 64 != 0 || ld < C || ld % 4 != 0)
        return FACL_E_SHAPE;
    if (!stacked || !classes || !protos || !proto_inv || !scale || !loss || !dstacked || !err || !ws) return FACL_E_NULL;
    if (((uintptr_t)stacked | (uintptr_t)protos | (uintptr_t)proto_inv | (uintptr_t)scale | (uintptr_t)dstacked | (uintptr_t)ws) & 15)
        return FACL_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    const int blocks = pn_blocks(M);
    if (int e = facl_launch_dynamic_lds<k_proto_nce, PN_LDS_MAX>(dim3((unsigned)blocks), dim3(PN_THREADS), (int)pn_lds_bytes(C, K), st, stacked,
                                                                 M, ld, C, B, classes, protos, proto_inv, scale, K, dstacked, part, err))
        return e;
    k_proto_finish<<<1, 64, 0, st>>>(part, blocks, M, loss);
    return facl_launch_status();
}
