// Weighted k-nearest-neighbour evaluation of frozen features: cosine top-k of every query row against a bank of
// rows, as a similarity GEMM on the fp16x3 exact split (common.h) whose epilogue keeps a running top-k per query, so the
// (nq, nb) similarity matrix never reaches HBM; and the exp(s / T)-weighted class vote over the k neighbours.
//
//   k_knn_rowinfo   one wave per row of q / x: sum of squares in fp64 and max|x| -> the row's power-of-two operand scale
//                   `sc` (max scaled into [2^13, 2^14)) and `post` = 1 / (max(||x||, 1e-12) * sc), the factor the epilogue
//                   applies.  No normalised copy of either operand exists.
//   k_knn_topk      workgroup = 128 queries x a contiguous range of 128-row bank tiles (grid.y = bank splits); wave w owns
//                   queries 32w..32w+31 against all 128 columns of a tile (1 x 4 MFMA tiles of 32x32), accumulates over all
//                   of C, then filters its accumulators against each query's current k-th entry and inserts the survivors
//                   into the query's sorted list in LDS (lane e = entry e).  The lists of a wave's 32 queries are private to
//                   that wave: no barrier and no atomic takes part in the selection.
//   k_knn_merge     one wave per query: merges the `splits` partial lists with the same insertion.
// Order: (similarity descending, bank index ascending) is a TOTAL order and every list is the k best of what it has seen under
// that order, so the result does not depend on the order of insertion, on the split count or on the run.
#include "common.h"
#include <limits.h>

namespace {

constexpr int KBK = 32;                        // contraction depth of one stage
constexpr int KROW = KBK + 8;                  // fp16 elements per LDS row (80 B: conflict-free b128 fragment reads)
constexpr int KBM = 128, KBN = 128;            // queries x bank rows per tile
constexpr int KPLANE = KBM * KROW;             // one fp16 plane of one operand (elements)
constexpr int KOPER_BYTES = 4 * KPLANE * 2;    // A hi, A lo, B hi, B lo
constexpr int KINFO_BYTES = 4 * KBM * 4;       // postq, self, k-th value, k-th index per query
constexpr int KMAX = 64;
constexpr int KTARGET_WGS = 512;               // two workgroups per CU on 256 CUs

struct KnnArgs {
    const float* q; const float* x;
    int nq, nb, C, ldq, ldx, k;
    const int* self_idx;
    const float* scq; const float* postq; const float* scb; const float* postb;
    float* pv; int* pi;                        // lists: row stride splits * k
    int splits, tiles_per_split, final;
};

__device__ __forceinline__ bool knn_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// Insert the wave-uniform candidate (v, col) into the sorted list LV / LI of k entries (lane e = entry e); `thrv` / `thri`
// receive the new k-th entry.  All 64 lanes call.
__device__ __forceinline__ void knn_insert(volatile float* LV, volatile int* LI, int k, float v, int col,
                                           volatile float* thrv, volatile int* thri) {
    const int e = lane_id();
    const bool in = e < k;
    const float ev = in ? LV[e] : -INFINITY;
    const int ei = in ? LI[e] : INT_MAX;
    const unsigned long long m = __ballot(in && knn_better(ev, ei, v, col));
    const int pos = __popcll(m);                                         // the entries ahead of the candidate are a prefix
    if (pos >= k) return;
    const float pv = __shfl_up(ev, 1, 64);
    const int pi = __shfl_up(ei, 1, 64);
    if (in && e >= pos) {
        const float nv = e == pos ? v : pv;
        const int ni = e == pos ? col : pi;
        LV[e] = nv; LI[e] = ni;
        if (e == k - 1) { *thrv = nv; *thri = ni; }
    }
}

__global__ __launch_bounds__(256) void k_knn_rowinfo(const float* __restrict__ x, int n, int C, int ld,
                                                     float* __restrict__ sc, float* __restrict__ post) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
    if (row >= n) return;
    const float4* p = reinterpret_cast<const float4*>(x + (size_t)row * ld);
    double ss = 0.0;
    float mx = 0.f;
    for (int i = lane; i < C / 4; i += 64) {
        const float4 v = p[i];
        ss += (double)v.x * v.x; ss += (double)v.y * v.y; ss += (double)v.z * v.z; ss += (double)v.w * v.w;
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    ss = wave_sum_f64(ss);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) {
        const float s = pow2_biased(h3_se(__float_as_uint(mx)));
        const double nrm = sqrt(ss);
        sc[row] = s;
        post[row] = (float)(1.0 / ((nrm > 1e-12 ? nrm : 1e-12) * (double)s));      // F.normalize: x / max(||x||, eps)
    }
}

__global__ __launch_bounds__(256, 2) void k_knn_topk(KnnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    unsigned short* const sA = reinterpret_cast<unsigned short*>(dsm);
    unsigned short* const sB = sA + 2 * KPLANE;
    float* const s_postq = reinterpret_cast<float*>(dsm + KOPER_BYTES);
    int* const s_self = reinterpret_cast<int*>(s_postq + KBM);
    volatile float* const s_thrv = reinterpret_cast<float*>(s_self + KBM);
    volatile int* const s_thri = reinterpret_cast<int*>(const_cast<float*>(s_thrv) + KBM);
    volatile float* const s_lv = reinterpret_cast<float*>(dsm + KOPER_BYTES + KINFO_BYTES);
    volatile int* const s_li = reinterpret_cast<int*>(const_cast<float*>(s_lv) + KBM * g.k);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, q = lane & 31;
    const int k = g.k;
    const int i0 = blockIdx.x * KBM;
    const int z = blockIdx.y;
    const int nbt = (g.nb + KBN - 1) / KBN;
    const int t0 = z * g.tiles_per_split;
    const int t1 = t0 + g.tiles_per_split < nbt ? t0 + g.tiles_per_split : nbt;
    const int KS = g.C / KBK;
    const int S = (t1 - t0) * KS;

    // the wave's own 32 queries: empty lists, thresholds, epilogue factor, excluded bank row
    for (int r = 0; r < 32; ++r) {
        const int row = 32 * wave + r;
        if (lane < k) { s_lv[row * k + lane] = -INFINITY; s_li[row * k + lane] = INT_MAX; }
    }
    if (lane < 32) {
        const int row = 32 * wave + lane;
        const int gr = i0 + row < g.nq ? i0 + row : g.nq - 1;
        s_postq[row] = g.postq[gr];
        s_self[row] = g.self_idx ? g.self_idx[gr] : -1;
        s_thrv[row] = -INFINITY; s_thri[row] = INT_MAX;
    }

    // staging: thread t loads k-chunk 4 * (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of each operand
    const int kc = 4 * (tid & 7), r0 = tid >> 3;
    const float* pa[4];
    float sca[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int row = i0 + r0 + 32 * i;
        row = row < g.nq ? row : g.nq - 1;
        pa[i] = g.q + (size_t)row * g.ldq + kc;
        sca[i] = g.scq[row];
    }
    float4 ra[4], rb[4];
    float scb[4];
    unsigned pka[16], pkb[16];
    auto fetch = [&](int s) {
        const int t = t0 + s / KS, k0 = (s % KS) * KBK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = *reinterpret_cast<const float4*>(pa[i] + k0);
            int row = t * KBN + r0 + 32 * i;
            row = row < g.nb ? row : g.nb - 1;
            rb[i] = *reinterpret_cast<const float4*>(g.x + (size_t)row * g.ldx + kc + k0);
            scb[i] = g.scb[row];
        }
    };
    auto split = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            split_pair_h(ra[i].x * sca[i], ra[i].y * sca[i], pka[4 * i], pka[4 * i + 2]);
            split_pair_h(ra[i].z * sca[i], ra[i].w * sca[i], pka[4 * i + 1], pka[4 * i + 3]);
            split_pair_h(rb[i].x * scb[i], rb[i].y * scb[i], pkb[4 * i], pkb[4 * i + 2]);
            split_pair_h(rb[i].z * scb[i], rb[i].w * scb[i], pkb[4 * i + 1], pkb[4 * i + 3]);
        }
    };
    auto write = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (r0 + 32 * i) * KROW + kc;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                *reinterpret_cast<uint2*>(sA + p * KPLANE + o) = make_uint2(pka[4 * i + 2 * p], pka[4 * i + 2 * p + 1]);
                *reinterpret_cast<uint2*>(sB + p * KPLANE + o) = make_uint2(pkb[4 * i + 2 * p], pkb[4 * i + 2 * p + 1]);
            }
        }
    };
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    auto mfma_block = [&](int kk) {
        f16x8h af[2], bf[4][2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            af[p] = *reinterpret_cast<const f16x8h*>(sA + p * KPLANE + (32 * wave + q) * KROW + 16 * kk + 8 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int p = 0; p < 2; ++p)
                bf[b][p] = *reinterpret_cast<const f16x8h*>(sB + p * KPLANE + (32 * b + q) * KROW + 16 * kk + 8 * h);
        constexpr int HA[3] = FACL_H3_PA, HB[3] = FACL_H3_PB;           // smallest terms first: (lo,hi) (hi,lo) (hi,hi)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] = MFMA_F16(af[HA[t]], bf[b][HB[t]], acc[b]);
    };

    if (S > 0) {
        fetch(0);
        split();
        write();
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int sn = s + 1 < S ? s + 1 : s;                            // the last stage re-reads its own tile: harmless
        fetch(sn);
        __builtin_amdgcn_sched_barrier(0);
        mfma_block(0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_block(1);
        split();
        __syncthreads();
        write();
        __syncthreads();
        if ((s + 1) % KS != 0) continue;                                 // workgroup-uniform
        // ---- the tile is complete: filter against each query's k-th entry, insert the survivors (wave-private lists)
        const int j0 = (t0 + s / KS) * KBN;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = j0 + 32 * b + q;
            const float pb = g.postb[col < g.nb ? col : g.nb - 1];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * wave + rowmap(r, h);
                const float v = (acc[b][r] * s_postq[row]) * pb;
                acc[b][r] = 0.f;
                const bool pass = col < g.nb && knn_better(v, col, s_thrv[row], s_thri[row]);
                unsigned long long m = __ballot(pass);
                while (m) {                                              // rare after the first tiles: k / (bank rows seen)
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float cv = __shfl(v, l, 64);
                    const int crow = 32 * wave + rowmap(r, l >> 5), ccol = j0 + 32 * b + (l & 31);
                    if (ccol == s_self[crow]) continue;
                    knn_insert(s_lv + crow * k, s_li + crow * k, k, cv, ccol, s_thrv + crow, s_thri + crow);
                }
            }
        }
    }
    // ---- the wave's lists -> partial (or final) lists
    for (int r = 0; r < 32; ++r) {
        const int row = 32 * wave + r, gr = i0 + row;
        if (gr < g.nq && lane < k) {
            const size_t o = ((size_t)gr * g.splits + z) * k + lane;
            const int idx = s_li[row * k + lane];
            g.pv[o] = s_lv[row * k + lane];
            g.pi[o] = (g.final && idx == INT_MAX) ? -1 : idx;
        }
    }
}

// one wave per query: the k best of its splits * k partial entries (the register-held list: lane e = entry e)
__global__ __launch_bounds__(256) void k_knn_merge(const float* __restrict__ pv, const int* __restrict__ pi, int nq, int k,
                                                   int splits, float* __restrict__ top_val, int* __restrict__ top_idx) {
    __shared__ float s_v[4][KMAX];
    __shared__ int s_i[4][KMAX];
    __shared__ float s_tv[4];
    __shared__ int s_ti[4];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int row = blockIdx.x * 4 + w;
    if (row >= nq) return;
    volatile float* LV = s_v[w];
    volatile int* LI = s_i[w];
    volatile float* tv = &s_tv[w];
    volatile int* ti = &s_ti[w];
    LV[lane] = -INFINITY; LI[lane] = INT_MAX;
    if (lane == 0) { *tv = -INFINITY; *ti = INT_MAX; }
    const int n = splits * k;
    const float* v = pv + (size_t)row * n;
    const int* ix = pi + (size_t)row * n;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        const float cv = c < n ? v[c] : -INFINITY;
        const int ci = c < n ? ix[c] : INT_MAX;
        unsigned long long m = __ballot(knn_better(cv, ci, *tv, *ti));
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            knn_insert(LV, LI, k, __shfl(cv, l, 64), __shfl(ci, l, 64), tv, ti);
        }
    }
    if (lane < k) {
        const int idx = LI[lane];
        top_val[(size_t)row * k + lane] = LV[lane];
        top_idx[(size_t)row * k + lane] = idx == INT_MAX ? -1 : idx;
    }
}

// one wave per query: lane j holds neighbour j's weight exp(s_j * inv_T) and label; lane c, c + 64, ... sum the weights of
// their classes over j = 0..k-1 in that order (no atomics: the same bits every run), then the wave takes the argmax.
__global__ __launch_bounds__(256) void k_knn_vote(const float* __restrict__ top_val, const int* __restrict__ top_idx,
                                                  const int* __restrict__ labels, int nq, int nb, int k, int num_class,
                                                  float inv_T, int* __restrict__ pred, float* __restrict__ scores) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
    if (row >= nq) return;
    float w = 0.f;
    int lab = -1;
    if (lane < k) {
        const int idx = top_idx[(size_t)row * k + lane];
        if (idx >= 0 && idx < nb) {
            lab = labels[idx];
            w = expf(top_val[(size_t)row * k + lane] * inv_T);
        }
    }
    float best = -INFINITY;
    int bc = INT_MAX;
    for (int c = lane; c < num_class + 63 - (num_class + 63) % 64; c += 64) {     // whole wave in every iteration (shuffles)
        float s = 0.f;
        for (int j = 0; j < k; ++j) {
            const float wj = __shfl(w, j, 64);
            const int lj = __shfl(lab, j, 64);
            if (lj == c) s += wj;
        }
        if (c < num_class) {
            if (scores) scores[(size_t)row * num_class + c] = s;
            if (s > best) { best = s; bc = c; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (oc != INT_MAX && (bc == INT_MAX || ob > best || (ob == best && oc < bc))) { best = ob; bc = oc; }
    }
    if (lane == 0) pred[row] = bc == INT_MAX ? 0 : bc;
}

inline int knn_splits(int nq, int nb, int* tiles_per_split) {
    const long long nqt = ((long long)nq + KBM - 1) / KBM, nbt = ((long long)nb + KBN - 1) / KBN;
    long long want = KTARGET_WGS / nqt;
    want = want < 1 ? 1 : (want > nbt ? nbt : want);
    const long long tps = (nbt + want - 1) / want;
    if (tiles_per_split) *tiles_per_split = (int)tps;
    return (int)((nbt + tps - 1) / tps);
}

inline size_t knn_rowinfo_bytes(int nq, int nb) { return (((size_t)nq + (size_t)nb) * 8 + 255) & ~(size_t)255; }

inline bool knn_shape_ok(int nq, int nb, int k) { return nq >= 1 && nb >= 1 && k >= 1 && k <= KMAX; }

}  // namespace

extern "C" int64_t facl_knn_ws_bytes(int nq, int nb, int k) {
    if (!knn_shape_ok(nq, nb, k)) return FACL_E_SHAPE;
    const int splits = knn_splits(nq, nb, nullptr);
    return (int64_t)(knn_rowinfo_bytes(nq, nb) + (splits > 1 ? (size_t)nq * splits * k * 8 : 0));
}

extern "C" int facl_knn_topk(const float* q, int nq, int ldq, const float* x, int nb, int ldx, int C, int k,
                             const int* self_idx, float* top_val, int* top_idx, void* ws, void* stream) {
    if (!knn_shape_ok(nq, nb, k) || C < 64 || C % 64 != 0 || ldq < C || ldx < C || ldq % 4 != 0 || ldx % 4 != 0)
        return FACL_E_SHAPE;
    if ((long long)nb - (self_idx ? 1 : 0) < k) return FACL_E_SHAPE;
    if (!q || !x || !top_val || !top_idx || !ws) return FACL_E_NULL;
    if (((uintptr_t)q | (uintptr_t)x | (uintptr_t)ws) & 15) return FACL_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    KnnArgs g;
    g.q = q; g.x = x; g.nq = nq; g.nb = nb; g.C = C; g.ldq = ldq; g.ldx = ldx; g.k = k;
    g.self_idx = self_idx;
    float* f = reinterpret_cast<float*>(ws);
    float* scq = f; float* postq = f + nq; float* scb = f + 2 * (size_t)nq; float* postb = scb + nb;
    g.scq = scq; g.postq = postq; g.scb = scb; g.postb = postb;
    g.splits = knn_splits(nq, nb, &g.tiles_per_split);
    g.final = g.splits == 1;
    if (g.final) { g.pv = top_val; g.pi = top_idx; }
    else {
        g.pv = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + knn_rowinfo_bytes(nq, nb));
        g.pi = reinterpret_cast<int*>(g.pv + (size_t)nq * g.splits * k);
    }
    const int lds = KOPER_BYTES + KINFO_BYTES + KBM * k * 8;
    k_knn_rowinfo<<<(nq + 3) / 4, 256, 0, st>>>(q, nq, C, ldq, scq, postq);
    k_knn_rowinfo<<<(nb + 3) / 4, 256, 0, st>>>(x, nb, C, ldx, scb, postb);
    // the candidate lists grow with k: the attribute covers k = KMAX
    if (int e = facl_launch_dynamic_lds<k_knn_topk, KOPER_BYTES + KINFO_BYTES + KBM * KMAX * 8>(dim3((nq + KBM - 1) / KBM, g.splits), dim3(256),
                                                                                                lds, st, g)) return e;
    if (!g.final) k_knn_merge<<<(nq + 3) / 4, 256, 0, st>>>(g.pv, g.pi, nq, k, g.splits, top_val, top_idx);
    return facl_launch_status();
}

extern "C" int facl_knn_vote(const float* top_val, const int* top_idx, const int* labels, int nq, int nb, int k, int num_class,
                             float inv_T, int* pred, float* scores, void* stream) {
    if (!knn_shape_ok(nq, nb, k) || num_class < 1 || num_class > 1024) return FACL_E_SHAPE;
    if (!top_val || !top_idx || !labels || !pred) return FACL_E_NULL;
    k_knn_vote<<<(nq + 3) / 4, 256, 0, (hipStream_t)stream>>>(top_val, top_idx, labels, nq, nb, k, num_class, inv_T, pred, scores);
    return facl_launch_status();
}
