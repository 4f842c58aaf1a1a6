// Spherical k-means over frozen features: the centroid update of one Lloyd iteration.  The assignment step is
// facl_knn_topk (knn.hip) with the centroids as the bank and k = 1; it normalises both operands per row itself, so the centroids
// kept here are the UN-normalised sums  cent[c] = sum over the rows i of cluster c of x_i / max(||x_i||, 1e-12).
//
//   k_cluster_row_inv  one wave per row: sum of squares in fp64 through the shared row body (norm_rows.h), inv = fp32(1 / max(||x||, eps)).
//                      Once per clustering: the rows do not change between iterations.
//   k_cluster_plan     one workgroup: checks the label boundaries `offs` and cuts every cluster into segments of CL_SEG rows of
//                      `order`; seg[c] = the first segment of cluster c (exclusive prefix sum, seg[K] = the number of segments).
//   k_cluster_partial  workgroup (one wave) = one segment x 256 columns: lane l owns four adjacent columns (one 16-byte load per row: the
//                      wave reads 1 KiB of a row, contiguous); the row index is uniform per workgroup and arrives through a scalar
//                      load of `order`; fp64 accumulators, rows in the order of `order`; the partial sums go to `ws` in fp64.
//   k_cluster_reduce   workgroup = one cluster x 256 columns: adds the cluster's segments in segment order, rounds ONCE to fp32.  A
//                      cluster without rows has no segment and its row of `cent` is left as it is.
// Determinism: no floating-point atomic; every sum runs in an order fixed by (n, order, offs) and CL_SEG alone, so two runs give
// the same bits.  x_ij * inv_i is exact in fp64 (24 x 24 significand bits), hence the only roundings are fp64 additions and the
// final one to fp32.  The one atomic is the integer OR that raises `err`.
// Robustness: an entry of `order` outside [0, n) never forms an address (the row is skipped, err |= 1); boundaries that are not
// 0 = offs[0] <= ... <= offs[K] = n plan no segment at all (err |= 2), so neither `order` nor `ws` is ever indexed out of bounds.
#include "common.h"
#include "norm_rows.h"

namespace {

constexpr int CL_SEG = 128;                    // rows of one segment
constexpr int CL_COLS = 256;                   // columns of one workgroup: 64 lanes x 4
constexpr int CL_UNROLL = 8;                   // rows in flight per wave (8 KiB)
constexpr int CL_KMAX = 1024;                  // facl_knn_vote's class limit
constexpr int CL_E_ORDER = 1, CL_E_OFFS = 2;

__global__ __launch_bounds__(256) void k_cluster_row_inv(const float* __restrict__ x, int n, int ld, int C, float* __restrict__ inv) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
    if (row >= n) return;                                                              // wave-uniform
    const float4* x4 = reinterpret_cast<const float4*>(x + (size_t)row * ld);
    double ss = 0.0;
    for (int c = lane; c < C / 4; c += 64) nr_acc_sq(ss, x4[c]);
    ss = wave_sum_f64(ss);
    if (lane == 0) inv[row] = (float)nr_inv_norm(ss);
}

__global__ __launch_bounds__(CL_KMAX) void k_cluster_plan(const int* __restrict__ offs, int n, int K, int* __restrict__ seg,
                                                          int* __restrict__ err) {
    __shared__ int s_wave[CL_KMAX / 64];
    const int c = threadIdx.x, lane = lane_id(), wave = c >> 6;
    int cnt = 0, bad = 0;
    if (c < K) {
        const int lo = offs[c], hi = offs[c + 1];
        bad = lo < 0 || hi > n || hi < lo || (c == 0 && lo != 0) || (c == K - 1 && hi != n);
        cnt = bad ? 0 : (hi - lo + CL_SEG - 1) / CL_SEG;
    }
    bad = __syncthreads_or(bad);
    if (bad) {                                                                         // workgroup-uniform: no segment at all
        if (c < K) seg[c + 1] = 0;
        if (c == 0) { seg[0] = 0; atomicOr(err, CL_E_OFFS); }
        return;
    }
    int v = cnt;                                                                       // inclusive scan: wave, then the waves in order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    if (c < K) seg[c + 1] = base + v;
    if (c == 0) seg[0] = 0;
}

// the cluster of segment s: the c with seg[c] <= s < seg[c + 1] (clusters without rows have seg[c] == seg[c + 1]); s < seg[K]
__device__ __forceinline__ int cluster_of_segment(const int* __restrict__ seg, int K, int s) {
    int lo = 0, hi = K;                                                                // seg[lo] <= s < seg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void k_cluster_partial(const float* __restrict__ x, int n, int ld, int C, const float* __restrict__ inv,
                                                        const int* __restrict__ order, const int* __restrict__ offs, int K,
                                                        const int* __restrict__ seg, int colblocks, double* __restrict__ part,
                                                        int* __restrict__ err) {
    // the column block runs fastest: workgroups that are dispatched together read adjacent KiBs of the SAME rows
    const int s = blockIdx.x / colblocks, cb = blockIdx.x - s * colblocks;
    if (s >= seg[K]) return;                                                           // workgroup-uniform: the grid is an upper bound
    const int c = cluster_of_segment(seg, K, s);
    const int r0 = offs[c] + (s - seg[c]) * CL_SEG;
    const int end = offs[c + 1], r1 = r0 + CL_SEG < end ? r0 + CL_SEG : end;           // the plan checked 0 <= offs[c] <= offs[c+1] <= n
    const int col = (cb * 64 + lane_id()) * 4;
    const bool live = col < C;
    const float* xc = x + (live ? col : 0);                                            // a lane past C reads column 0 and stores nothing
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int bad = 0;
    // Branch-free, so that the loads of CL_UNROLL rows are in flight together (with a branch per row the compiler waits for every
    // load before it issues the next).  A position past the segment's end repeats its last one, and an index outside [0, n) is
    // replaced by row 0 (n >= 1) BEFORE any address is formed; what such a slot loads is dropped by the selects below.
    for (int r = r0; r < r1; r += CL_UNROLL) {
        int idx[CL_UNROLL], raw[CL_UNROLL];
        bool ok[CL_UNROLL];
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) raw[u] = order[r + u < r1 ? r + u : r1 - 1];   // uniform addresses: scalar loads
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) {
            const bool in = r + u < r1;
            const int i = raw[u];
            ok[u] = in && (unsigned)i < (unsigned)n;
            bad |= in && !ok[u];
            idx[u] = ok[u] ? i : 0;
        }
        float4 v[CL_UNROLL];
        float w[CL_UNROLL];
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) {
            w[u] = inv[idx[u]];
            v[u] = *reinterpret_cast<const float4*>(xc + (size_t)idx[u] * ld);
        }
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) {                                          // the sums, in row order; a skipped slot adds 0
            const double wi = ok[u] ? (double)w[u] : 0.0;
            a0 += (double)(ok[u] ? v[u].x : 0.f) * wi; a1 += (double)(ok[u] ? v[u].y : 0.f) * wi;
            a2 += (double)(ok[u] ? v[u].z : 0.f) * wi; a3 += (double)(ok[u] ? v[u].w : 0.f) * wi;
        }
    }
    if (live) {
        double* p = part + (size_t)s * C + col;
        *reinterpret_cast<double2*>(p) = make_double2(a0, a1);
        *reinterpret_cast<double2*>(p + 2) = make_double2(a2, a3);
    }
    if (bad && threadIdx.x == 0) atomicOr(err, CL_E_ORDER);
}

__global__ __launch_bounds__(64) void k_cluster_reduce(const double* __restrict__ part, const int* __restrict__ seg, int C,
                                                       float* __restrict__ cent) {
    const int c = blockIdx.x;
    const int s0 = seg[c], s1 = seg[c + 1];
    const int col = (blockIdx.y * 64 + lane_id()) * 4;
    if (s0 >= s1 || col >= C) return;                                                  // no rows: the centroid stays
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int s = s0; s < s1; ++s) {
        const double* p = part + (size_t)s * C + col;
        const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
        a0 += lo.x; a1 += lo.y; a2 += hi.x; a3 += hi.y;
    }
    *reinterpret_cast<float4*>(cent + (size_t)c * C + col) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

inline long long cluster_slots(int n, int K) { return (long long)n / CL_SEG + K; }     // >= sum over c of ceil(size_c / CL_SEG)

// the partial launch is one linear grid of slots x column blocks: it has to fit 31 bits
inline bool cluster_rows_ok(int n, int ldx, int C) { return n >= 1 && C >= 64 && C % 64 == 0 && ldx >= C && ldx % 4 == 0; }
inline bool cluster_grid_ok(int n, int K, int C) { return cluster_slots(n, K) * ((C + CL_COLS - 1) / CL_COLS) <= 0x7fffffffLL; }

inline size_t cluster_plan_bytes(int K) { return (((size_t)K + 1) * 4 + 255) & ~(size_t)255; }

}  // namespace

extern "C" int64_t facl_cluster_ws_bytes(int n, int K, int C) {
    if (n < 1 || K < 1 || K > CL_KMAX || C < 64 || C % 64 != 0 || !cluster_grid_ok(n, K, C)) return FACL_E_SHAPE;
    return (int64_t)(cluster_plan_bytes(K) + (size_t)cluster_slots(n, K) * (size_t)C * 8);
}

extern "C" int facl_cluster_row_inv(const float* x, int n, int ldx, int C, float* inv, void* stream) {
    if (!cluster_rows_ok(n, ldx, C)) return FACL_E_SHAPE;
    if (!x || !inv) return FACL_E_NULL;
    if ((uintptr_t)x & 15) return FACL_E_ALIGN;
    k_cluster_row_inv<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, n, ldx, C, inv);
    return facl_launch_status();
}

extern "C" int facl_cluster_sums(const float* x, int n, int ldx, int C, const float* inv, const int32_t* order, const int32_t* offs,
                                 int K, float* cent, int32_t* err, void* ws, void* stream) {
    if (!cluster_rows_ok(n, ldx, C) || K < 1 || K > CL_KMAX || !cluster_grid_ok(n, K, C)) return FACL_E_SHAPE;
    if (!x || !inv || !order || !offs || !cent || !err || !ws) return FACL_E_NULL;
    if (((uintptr_t)x | (uintptr_t)cent | (uintptr_t)ws) & 15) return FACL_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    int* seg = reinterpret_cast<int*>(ws);
    double* part = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(ws) + cluster_plan_bytes(K));
    const unsigned colblocks = (unsigned)((C + CL_COLS - 1) / CL_COLS);
    k_cluster_plan<<<1, CL_KMAX, 0, st>>>(offs, n, K, seg, err);
    k_cluster_partial<<<(unsigned)(cluster_slots(n, K) * colblocks), 64, 0, st>>>(x, n, ldx, C, inv, order, offs, K, seg, (int)colblocks,
                                                                                 part, err);
    k_cluster_reduce<<<dim3((unsigned)K, colblocks), 64, 0, st>>>(part, seg, C, cent);
    return facl_launch_status();
}
