// Global / circle InfoNCE-style losses on a similarity matrix (utils_my.py:53-116 =
// cn3d_train_motion_GL.py:265-316), forward value and d(loss)/d(sim) in one kernel.
//
// sim = anchors @ keys^T has J = G*Bk key columns (column j belongs to clip j % Bk); a clip n has nA anchor rows (1 for the
// global loss, G-1 for the circle loss) and nS positive slots (G resp. G-1).  Reference semantics:
//   * same-clip columns are MULTIPLIED BY 0 (utils_my.py:72,106), i.e. they stay in the softmax as exp(0);
//   * all nA anchor rows of a clip share ONE negative set (the `repeat` at :74 / :108), so
//     lse[n] = log sum_{i,j} exp(sim'[row(i, n), j]);
//   * logits[s] = [pos[s,n] | negatives], label 0, CE = mean over the B clips, summed over the slots s.
// pos[s,n] is read BEFORE masking: the positive key is a same-clip column.
// Per clip: loss_n = sum_s (logaddexp(pos, lse) - pos) / B;   dsim follows by the chain rule.
#include <type_traits>
#include "common.h"
#include "norm_rows.h"

int facl_reduce_rows(const double* part, int rows, int V, double* out, hipStream_t st);
extern "C" int64_t facl_ws_bytes(void);

namespace {

__device__ __forceinline__ float block_reduce_max(float v, float* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, sm[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_reduce_sum(double v, double* sm) {
    v = wave_sum_f64(v);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sm[w];
    __syncthreads();
    return r;
}

// counts: exact, in the same fixed order as the sums above (sm: 16 words, e.g. block_reduce_max's floats)
__device__ __forceinline__ int block_reduce_count(int v, int* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sm[w];
    __syncthreads();
    return r;
}

// One positive slot against the clip's log-sum-exp: t = logaddexp(pos, lse), sigma = exp(pos - t).  loss = t - pos is the slot's
// loss term, dlse = 1 - sigma its share of d/dlse, dpos = sigma - 1 its d/dpos; the caller accumulates and applies the 1/B.
struct SlotTerm { float loss, dlse, dpos; };
__device__ __forceinline__ SlotTerm slot_term(float pos, float lse) {
    const float t = fmaxf(pos, lse) + log1pf(__expf(-fabsf(pos - lse)));
    return {t - pos, 1.f - __expf(pos - t), __expf(pos - t) - 1.f};
}

// ---------------------------------------------------------------------------------------------------------------------
// Both losses of a step in ONE launch on ONE similarity matrix.  sim is ((G+1)*B, J) = [x ; x_global] @ keys^T: row
// block g < G holds view g of the local clips (row g*B + n), block G the clip-level embeddings x_global.  Workgroups
// 0..B-1 evaluate the global loss of clip n (anchor block G, one positive per view g in column g*Bk + clip), workgroups
// B..2B-1 the circle loss (anchor blocks order[0..G-2], positive of slot i in block order[i], column order[i+1]*Bk + clip;
// block order[G-1] is no anchor: its dsim row is zeroed here so that every row of dsim is written exactly once).
// No anchors gather, no positive-column index tensors and one similarity GEMM for both losses.
//
// MASK selects what a same-clip column is inside the log-sum-exp.  MASK_ZERO: the reference's rule above, the column is the
// value 0 and counts exp(0); since every clip has such a column, the running maximum may start at 0, an element past the end of
// the cached block may be loaded as 0, and every cached element may be summed.  MASK_EXCLUDE: the column is no member of the
// sum at all (negatives only), so none of the three holds: the maximum starts at -inf and masked / past-the-end elements are
// skipped by the maximum and by the sum (Bk >= 2: at least one negative exists).  In both modes the masked columns' dsim is 0
// and the positives are read before masking.
// MASK_CLASS: `exclude`, and beside the clip's own columns every column of a clip KNOWN to share the anchor's class leaves the
// sum (false-negative removal with labels): cls (Bk int32) holds one class id per key clip, >= 0 a class, < 0 unknown; column j
// is masked iff j % Bk == myclip || (cls[myclip] >= 0 && cls[j % Bk] == cls[myclip]).  The ids are only compared, never used
// as an index.  Here a clip may have NO negative (a batch of one class): mx = -inf and se = 0 give lse = -inf + log(0) = -inf,
// every slot's t = pos + log1p(exp(-inf)) = pos, so loss, dpos and dlse are exactly 0 and no exp(x - lse) is evaluated (every
// column is masked) -- the arithmetic below needs no special case.
// MASK_SUP: MASK_CLASS, and the cells it masks for a reason other than "own clip" -- the clip's CLASS CELLS C -- are positive
// slots as well, against the same lse: loss_n = sum_s term(pos_s) + w sum_{c in C} term(v_c) with w = pw * nS / |C| (nothing is
// added when |C| = 0), so the class cells enter through their mean term and weigh, at pw = 1, as much as the nS own slots.  A
// class cell's gradient is w dpos / B, its dlse share times w joins the own slots' in the coefficient of the negatives; |C| is
// a count and is not differentiated.  The class cells stay out of the maximum and the exp-sum; the own slots are reduced
// exactly as in the other modes, so with |C| = 0 everywhere every output has MASK_EXCLUDE's bits.  lse = -inf: slot_term gives
// exact zeros for the class cells too.  Internal to this file (facl_contrast_pair_sum_sup / _queue_sup); no mask_mode argument
// of the ABI takes it.
constexpr int MASK_ZERO = 0, MASK_EXCLUDE = 1, MASK_CLASS = 2, MASK_SUP = 3;

// jm = j % Bk, mycls = cls[myclip] (MASK_CLASS and MASK_SUP only)
template <int MASK>
__device__ __forceinline__ bool col_masked(int jm, int myclip, int mycls, const int* __restrict__ cls) {
    if constexpr (MASK >= MASK_CLASS) return jm == myclip || (mycls >= 0 && cls[jm] == mycls);
    else return jm == myclip;
}

// w = pw * nS / |C| of MASK_SUP, in fp64 from the fp32 weight and the two counts
__device__ __forceinline__ double sup_weight(float pw, int nS, int cells) { return (double)pw * (double)nS / (double)cells; }

// One loss of one clip: the circle loss (circle = 1) or the global loss of local clip n, key clip myclip = n + clip_offset.
// nA = anchor rows of the clip that feed its shared negative set, nS = its positive slots (kept as fields: as functions of
// (circle, G) at each use they changed the generated code of the pair and queue kernels).
struct PairSpec {
    int nA, nS, circle, G, B, Bk, J, myclip, n;
    const long long* order;
    __device__ __forceinline__ PairSpec(int circle, int n, int G, int B, int Bk, int J, int clip_offset, const long long* order)
        : nA(circle ? G - 1 : 1), nS(circle ? G - 1 : G), circle(circle), G(G), B(B), Bk(Bk), J(J), myclip(n + clip_offset), n(n),
          order(order) {}
    __device__ __forceinline__ int ord(int i) const {            // clamped: a corrupt entry cannot address outside sim / dsim
        const long long o = order[i];
        return o < 0 ? 0 : (o >= G ? G - 1 : (int)o);
    }
    __device__ __forceinline__ int row_block(int i) const { return circle ? ord(i) : G; }
    // slot s reads its positive from its own anchor row (circle) or from the one global row
    __device__ __forceinline__ size_t pos_index(int s) const {
        const int rb = row_block(circle ? s : 0);
        const int col = (circle ? ord(s + 1) : s) * Bk + myclip;
        return (size_t)(rb * B + n) * J + col;
    }
};

// 1024 threads per clip and the clip's nA x J similarities held in registers between the passes (one read of sim, no
// per-element integer modulo in the inner passes): the grid is only 2B workgroups, so the kernel is latency-bound and three
// streaming passes with 256 threads took 65 us for the circle loss at H.
constexpr int CK = 24;                      // cached values per thread: nA*J <= 24*1024

template <int MASK>
__global__ __launch_bounds__(1024) void k_contrast_pair_reg(const float* __restrict__ sim, int G, int B, int Bk, int J,
                                                           const long long* __restrict__ order, int clip_offset,
                                                           float* __restrict__ dsim, double* __restrict__ part,
                                                           const int* __restrict__ cls, float pw) {
    __shared__ float smf[16];
    __shared__ double smd[16];
    __shared__ int rb_s[1024];
    const int circle = blockIdx.x >= (unsigned)B;
    const PairSpec sp(circle, circle ? blockIdx.x - B : blockIdx.x, G, B, Bk, J, clip_offset, order);
    const int n = sp.n, myclip = sp.myclip, nA = sp.nA, nS = sp.nS;
    int mycls = -1;
    if constexpr (MASK >= MASK_CLASS) mycls = cls[myclip];
    if ((int)threadIdx.x < nA) rb_s[threadIdx.x] = sp.row_block(threadIdx.x);
    __syncthreads();
    const int total = nA * J;
    // Element e = tid + 1024 k of the (nA x J) block: row i = e / J, column j = e % J, and j % Bk for the same-clip mask.  The
    // divisions are taken ONCE per thread and advanced by increments (one wrap at most per step: 1024 % J < J): with a division
    // pair per element and pass -- 4 x 18 runtime divisions of ~35 instructions each -- this kernel was VALU-bound on its index
    // arithmetic (23.5 us on 64 workgroups); the offsets are kept for the write pass (bit 31 = masked column).
    const int di = 1024 / J, dj = 1024 - di * J, djm = dj % Bk, Jm = J % Bk;
    int wi = (int)threadIdx.x / J, wj = (int)threadIdx.x - wi * J, wjm = wj % Bk;
    const auto advance = [&](int& i, int& j, int& jm) {    // (row, column, column % Bk) of the element 1024 further on
        i += di; j += dj; jm += djm;
        if (j >= J) { j -= J; ++i; jm += Bk - Jm; }
        if (jm >= Bk) jm -= Bk;
        if (jm >= Bk) jm -= Bk;
    };
    float v[CK];
    unsigned off[CK];
    // MASK_CLASS: bit k = element k lies in a column of the anchor's known class.  The CK lookups run FIRST, in a pass of their
    // own over the same column index and without a condition (the index stays inside [0, Bk) past the end of the block too), so
    // that they are CK requests in flight at once: with the lookup inside the loop below every similarity load waited for its id,
    // CK round trips instead of one, +28 us per step at the headline size.
    // MASK_SUP: the same word; bit k of `cell` = element k is a class cell (same class, not the own clip): it is loaded, stays
    // out of the maximum and the sum (bit 31 of off) and becomes a positive slot once lse is known.
    unsigned same_cls = 0u, cell = 0u;
    if constexpr (MASK >= MASK_CLASS) {
        if (mycls >= 0) {                                  // workgroup-uniform
            int pi = wi, pj = wj, pjm = wjm;
#pragma unroll
            for (int k = 0; k < CK; ++k, advance(pi, pj, pjm)) same_cls |= (unsigned)(cls[pjm] == mycls) << k;
        }
    }
    float mx = MASK == MASK_ZERO ? 0.f : -INFINITY;        // zero: masked entries are 0, there is at least one
#pragma unroll
    for (int k = 0; k < CK; ++k, advance(wi, wj, wjm)) {
        const int e = threadIdx.x + k * 1024;
        float x = 0.f;                                     // beyond the end: behaves like a masked column
        off[k] = 0x80000000u;
        if (e < total) {
            const unsigned o = (unsigned)((rb_s[wi] * B + n) * J + wj);
            bool masked = wjm == myclip;
            if constexpr (MASK >= MASK_CLASS) masked = masked || ((same_cls >> k) & 1u);
            off[k] = masked ? (o | 0x80000000u) : o;
            if constexpr (MASK == MASK_SUP) {
                const bool c = wjm != myclip && ((same_cls >> k) & 1u);
                cell |= (unsigned)c << k;
                if (!masked || c) x = sim[o];
            } else {
                if (!masked) x = sim[o];
            }
        }
        v[k] = x;
        if (MASK == MASK_ZERO || !(off[k] >> 31)) mx = fmaxf(mx, x);
    }
    // the positives' similarities do not depend on the log-sum-exp: requested with the block, not behind two reductions
    float pos = 0.f;
    size_t ppos = 0;
    const bool has_pos = (int)threadIdx.x < nS;            // nS <= 1024: at most one per thread
    if (has_pos) { ppos = sp.pos_index(threadIdx.x); pos = sim[ppos]; }
    mx = block_reduce_max(mx, smf);
    double se = 0;
#pragma unroll
    for (int k = 0; k < CK; ++k)
        if (MASK == MASK_ZERO ? (int)threadIdx.x + k * 1024 < total : !(off[k] >> 31)) se += (double)__expf(v[k] - mx);
    se = block_reduce_sum(se, smd);
    const float lse = mx + (float)log(se);
    double loss_t = 0, dlse_t = 0;
    float dpos = 0.f;
    const float invB = 1.f / (float)B;
    if (has_pos) {
        const SlotTerm st = slot_term(pos, lse);
        loss_t += (double)st.loss;
        dlse_t += (double)st.dlse;
        dpos = st.dpos * invB;
    }
    double loss = block_reduce_sum(loss_t, smd);
    const double dlse_s = block_reduce_sum(dlse_t, smd);
    float dlse = (float)dlse_s * invB;
    float wB = 0.f;                                        // MASK_SUP: w / B, the factor on a class cell's dpos
    if constexpr (MASK == MASK_SUP) {
        int cn = 0;
        double ct = 0, cd = 0;
#pragma unroll
        for (int k = 0; k < CK; ++k)
            if ((cell >> k) & 1u) {
                const SlotTerm st = slot_term(v[k], lse);
                ++cn;
                ct += (double)st.loss;
                cd += (double)st.dlse;
                v[k] = st.dpos;                            // the cell's value has served: the write pass needs only this
            }
        cn = block_reduce_count(cn, reinterpret_cast<int*>(smf));
        if (cn > 0) {                                      // workgroup-uniform
            const double w = sup_weight(pw, nS, cn);
            loss += w * block_reduce_sum(ct, smd);
            dlse = (float)(dlse_s + w * block_reduce_sum(cd, smd)) * invB;
            wB = (float)w * invB;
        }
    }
#pragma unroll
    for (int k = 0; k < CK; ++k) {
        const int e = threadIdx.x + k * 1024;
        if (e < total) {
            float d = (off[k] >> 31) ? 0.f : dlse * __expf(v[k] - lse);
            if constexpr (MASK == MASK_SUP)
                if ((cell >> k) & 1u) d = wB * v[k];
            dsim[off[k] & 0x7fffffffu] = d;
        }
    }
    if (sp.circle) {                                       // the view that is no anchor: zero gradient row
        float* z = dsim + (size_t)(sp.ord(G - 1) * B + n) * J;
        for (int j = threadIdx.x; j < J; j += 1024) z[j] = 0.f;
    }
    __syncthreads();                                       // the positives overwrite zeros written just above
    if ((int)threadIdx.x < nS) dsim[ppos] = dpos;
    if (threadIdx.x == 0) part[2 * n + sp.circle] = loss * (double)invB;
}

// streaming form for shapes the register-cached kernel cannot hold ((G-1)*J > CK*1024 or G > 1024)
template <int MASK>
__global__ __launch_bounds__(256) void k_contrast_pair(const float* __restrict__ sim, int G, int B, int Bk, int J,
                                                       const long long* __restrict__ order, int clip_offset,
                                                       float* __restrict__ dsim, double* __restrict__ part,
                                                       const int* __restrict__ cls, float pw) {
    __shared__ float smf[4];
    __shared__ double smd[4];
    const int circle = blockIdx.x >= (unsigned)B;
    const PairSpec sp(circle, circle ? blockIdx.x - B : blockIdx.x, G, B, Bk, J, clip_offset, order);
    const int n = sp.n, myclip = sp.myclip, nA = sp.nA, nS = sp.nS;
    int mycls = -1;
    if constexpr (MASK >= MASK_CLASS) mycls = cls[myclip];
    float mx = MASK == MASK_ZERO ? 0.f : -INFINITY;
    for (int i = 0; i < nA; ++i) {
        const float* row = sim + (size_t)(sp.row_block(i) * B + n) * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            if constexpr (MASK == MASK_ZERO) mx = fmaxf(mx, (j % Bk == myclip) ? 0.f : row[j]);
            else if (!col_masked<MASK>(j % Bk, myclip, mycls, cls)) mx = fmaxf(mx, row[j]);
        }
    }
    mx = block_reduce_max(mx, smf);
    double se = 0;
    for (int i = 0; i < nA; ++i) {
        const float* row = sim + (size_t)(sp.row_block(i) * B + n) * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            if constexpr (MASK == MASK_ZERO) se += (double)__expf(((j % Bk == myclip) ? 0.f : row[j]) - mx);
            else if (!col_masked<MASK>(j % Bk, myclip, mycls, cls)) se += (double)__expf(row[j] - mx);
        }
    }
    se = block_reduce_sum(se, smd);
    const float lse = mx + (float)log(se);
    float dlse = 0.f;
    double loss = 0;
    for (int s = 0; s < nS; ++s) {
        const SlotTerm st = slot_term(sim[sp.pos_index(s)], lse);
        loss += (double)st.loss;
        dlse += st.dlse;
    }
    const float invB = 1.f / (float)B;
    float wB = 0.f;                                        // MASK_SUP: w / B, the factor on a class cell's dpos
    if constexpr (MASK == MASK_SUP) {                      // the class cells (see MASK_SUP above): one more strided pass
        int cn = 0;
        double ct = 0, cd = 0;
        if (mycls >= 0)                                    // workgroup-uniform
            for (int i = 0; i < nA; ++i) {
                const float* row = sim + (size_t)(sp.row_block(i) * B + n) * J;
                for (int j = threadIdx.x; j < J; j += 256) {
                    const int jm = j % Bk;
                    if (jm == myclip || cls[jm] != mycls) continue;
                    const SlotTerm st = slot_term(row[j], lse);
                    ++cn;
                    ct += (double)st.loss;
                    cd += (double)st.dlse;
                }
            }
        cn = block_reduce_count(cn, reinterpret_cast<int*>(smf));
        if (cn > 0) {                                      // workgroup-uniform
            const double w = sup_weight(pw, nS, cn);
            loss += w * block_reduce_sum(ct, smd);
            dlse = (float)((double)dlse + w * block_reduce_sum(cd, smd));
            wB = (float)w * invB;
        }
    }
    dlse *= invB;
    for (int i = 0; i < nA; ++i) {
        const size_t ro = (size_t)(sp.row_block(i) * B + n) * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            const int jm = j % Bk;
            float d = col_masked<MASK>(jm, myclip, mycls, cls) ? 0.f : dlse * __expf(sim[ro + j] - lse);
            if constexpr (MASK == MASK_SUP)
                if (jm != myclip && mycls >= 0 && cls[jm] == mycls) d = wB * slot_term(sim[ro + j], lse).dpos;
            dsim[ro + j] = d;
        }
    }
    if (sp.circle) {
        float* z = dsim + (size_t)(sp.ord(G - 1) * B + n) * J;
        for (int j = threadIdx.x; j < J; j += 256) z[j] = 0.f;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nS; s += 256) {
        const size_t pp = sp.pos_index(s);
        dsim[pp] = slot_term(sim[pp], lse).dpos * invB;
    }
    if (threadIdx.x == 0) part[2 * n + sp.circle] = loss * (double)invB;
}

// ---------------------------------------------------------------------------------------------------------------------
// Row pass in front of the similarity GEMM: n_r = x_r * s / max(||x_r||_2, 1e-12) (NORM) or n_r = x_r * s, with s = 1/sqrt(tau),
// so that n @ n^T is cos/tau resp. <.,.>/tau and the GEMMs and the loss launch see no temperature.  One wave per row, 16-byte
// loads; the sum of squares / the dot product in fp64 in the order of norm_rows.h (per lane, then the xor tree); every element
// is rounded once to fp32.  No LDS, no atomic: the same bits every run.
constexpr int LR_THREADS = 256, LR_WAVES = LR_THREADS / 64;

template <bool NORM>
__global__ __launch_bounds__(LR_THREADS) void k_loss_rows_fwd(const float* __restrict__ x, long long R, int C, float s,
                                                              float* __restrict__ n, float* __restrict__ inv_norm) {
    const long long row = (long long)blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;                                                            // wave-uniform
    const int lane = lane_id(), C4 = C >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + (size_t)row * C);
    float4* n4 = reinterpret_cast<float4*>(n + (size_t)row * C);
    double inv = 1.0;
    if constexpr (NORM) {
        double ss = 0.0;
        for (int c = lane; c < C4; c += 64) nr_acc_sq(ss, x4[c]);
        inv = nr_inv_norm(wave_sum_f64(ss));
    }
    const double sc = (double)s * inv;
    for (int c = lane; c < C4; c += 64) n4[c] = nr_scale_f64(x4[c], sc);
    if (lane == 0) inv_norm[row] = (float)inv;
}

// dx_r = s inv_r (dn_r - xh_r <dn_r, xh_r>) with the unit row xh_r = n_r / s, i.e. nr_project on (dn_r, n_r) with the dot
// product divided by s^2;  without normalisation dx_r = s dn_r.
template <bool NORM>
__global__ __launch_bounds__(LR_THREADS) void k_loss_rows_bwd(const float* __restrict__ dn, const float* __restrict__ n,
                                                              const float* __restrict__ inv_norm, long long R, int C, float s,
                                                              float* __restrict__ dx) {
    const long long row = (long long)blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;                                                            // wave-uniform
    const int lane = lane_id(), C4 = C >> 2;
    const float4* d4 = reinterpret_cast<const float4*>(dn + (size_t)row * C);
    float4* o4 = reinterpret_cast<float4*>(dx + (size_t)row * C);
    if constexpr (NORM) {
        const float4* n4 = reinterpret_cast<const float4*>(n + (size_t)row * C);
        double dot = 0.0;
        for (int c = lane; c < C4; c += 64) nr_acc_dot(dot, d4[c], n4[c]);
        dot = wave_sum_f64(dot) / ((double)s * (double)s);
        const double sc = (double)s * (double)inv_norm[row];
        for (int c = lane; c < C4; c += 64) o4[c] = nr_project(sc, d4[c], n4[c], dot);
    } else {
        for (int c = lane; c < C4; c += 64) o4[c] = nr_scale_f64(d4[c], (double)s);
    }
}

// dst[r][:] = src[r][:] * (r < R1 ? *g1 : *g2): the chain rule of the two loss values onto the shared d/dsim matrix
template <typename V>
__global__ __launch_bounds__(256) void k_scale_rows2(const V* __restrict__ src, V* __restrict__ dst, long long n,
                                                     long long split, const float* __restrict__ g1,
                                                     const float* __restrict__ g2) {
    const float a = *g1, b = *g2;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float g = i < split ? a : b;
        if constexpr (sizeof(V) == 16) {
            float4 v = src[i];
            v.x *= g; v.y *= g; v.z *= g; v.w *= g;
            dst[i] = v;
        } else {
            dst[i] = src[i] * g;
        }
    }
}

// The fp32 values the training loop works with, from the per-clip partials: losses32 = [loss_c, loss_circle, loss_circle + loss_c]
// (the sum in fp32, exactly the reference's `loss = loss_circle + loss_c` on the two fp32 losses, cn3d_train_motion_GL.py:329)
// -- one single-workgroup launch instead of a reduction, a dtype cast and an add.
__global__ __launch_bounds__(64) void k_loss_finish(const double* __restrict__ part, int B, double* __restrict__ losses,
                                                    float* __restrict__ losses32) {
    double c = 0, o = 0;
    for (int n = threadIdx.x; n < B; n += 64) { c += part[2 * n]; o += part[2 * n + 1]; }
    c = wave_sum_f64(c);
    o = wave_sum_f64(o);
    if (threadIdx.x == 0) {
        losses[0] = c; losses[1] = o;
        const float fc = (float)c, fo = (float)o;
        losses32[0] = fc; losses32[1] = fo; losses32[2] = fo + fc;
    }
}

int finish_losses(const void* part, int B, double* losses, float* losses32, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(64), 0, st, (const double*)part, B, losses, losses32);
    return facl_launch_status();
}

// The shapes every pair entry takes.  have_ids: the class ids MASK_CLASS / MASK_SUP read were passed; the entries with a
// mask_mode argument pass none, so modes 2 and 3 are no modes of theirs.
bool pair_shape_ok(int G, int B, int Bk, int J, int clip_offset, int mask_mode, bool have_ids) {
    if (G < 2 || B < 1 || Bk < 1 || J != G * Bk) return false;
    if (clip_offset < 0 || clip_offset + B > Bk) return false;               // the local clips must be columns of the keys
    if (mask_mode != MASK_ZERO && mask_mode != MASK_EXCLUDE && !((mask_mode == MASK_CLASS || mask_mode == MASK_SUP) && have_ids)) return false;
    return mask_mode == MASK_ZERO || Bk >= 2;                                // one key clip: no negative exists
}

// f(integral_constant<int, MASK>) for a mask mode that pair_shape_ok has admitted
template <class F>
void with_mask(int mask_mode, F&& f) {
    if (mask_mode == MASK_ZERO) f(std::integral_constant<int, MASK_ZERO>{});
    else if (mask_mode == MASK_EXCLUDE) f(std::integral_constant<int, MASK_EXCLUDE>{});
    else if (mask_mode == MASK_CLASS) f(std::integral_constant<int, MASK_CLASS>{});
    else f(std::integral_constant<int, MASK_SUP>{});
}

// the weight of MASK_SUP's class cells: finite and > 0
inline bool pos_weight_ok(float pw) { return pw > 0.f && pw <= 3.402823466e38f; }

// shape checks and launch of the pair kernels: per-clip partial losses [loss_c, loss_circle] into ws, d/dsim into dsim
int launch_pair(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset, int mask_mode, float* dsim,
                void* ws, hipStream_t st, const int32_t* cls = nullptr, float pw = 0.f) {
    if (!pair_shape_ok(G, B, Bk, J, clip_offset, mask_mode, cls != nullptr)) return FACL_E_SHAPE;
    const bool reg = (long long)(G - 1) * J <= (long long)CK * 1024 && G <= 1024 && (long long)(G + 1) * B * J < 0x7fffffffLL;
    with_mask(mask_mode, [&](auto m) {
        constexpr int MASK = decltype(m)::value;
        if (reg)
            hipLaunchKernelGGL(k_contrast_pair_reg<MASK>, dim3(2 * B), dim3(1024), 0, st, sim, G, B, Bk, J, (const long long*)order,
                               clip_offset, dsim, (double*)ws, (const int*)cls, pw);
        else
            hipLaunchKernelGGL(k_contrast_pair<MASK>, dim3(2 * B), dim3(256), 0, st, sim, G, B, Bk, J, (const long long*)order,
                               clip_offset, dsim, (double*)ws, (const int*)cls, pw);
    });
    return facl_launch_status();
}

// facl_contrast_pair_sum_mask / _cls / _sup behind their NULL checks
int pair_sum(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset, int mask_mode, const int32_t* cls,
             float* dsim, double* losses, float* losses32, void* ws, void* stream, float pw = 0.f) {
    if (!sim || !order || !dsim || !losses || !losses32 || !ws) return FACL_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_pair(sim, G, B, Bk, J, order, clip_offset, mask_mode, dsim, ws, st, cls, pw);
    return rc ? rc : finish_losses(ws, B, losses, losses32, st);
}

inline bool loss_rows_ok(int64_t R, int C, int normalize, float s) {
    return R >= 1 && (R + LR_WAVES - 1) / LR_WAVES <= 0x7fffffffLL && C >= 4 && C % 4 == 0 && (normalize == 0 || normalize == 1) &&
           s > 0.f && s <= 3.402823466e38f;
}
}  // namespace

extern "C" int facl_contrast_pair(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                  float* dsim, double* losses /* [loss_c, loss_circle] */, void* ws, void* stream) {
    if (!sim || !order || !dsim || !losses || !ws) return FACL_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_pair(sim, G, B, Bk, J, order, clip_offset, MASK_ZERO, dsim, ws, st);
    if (rc) return rc;
    return facl_reduce_rows((const double*)ws, B, 2, losses, st);
}

// facl_contrast_pair finished by k_loss_finish, with the mask mode of the same-clip columns as an argument (0 = zero, 1 = exclude)
extern "C" int facl_contrast_pair_sum_mask(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                           int mask_mode, float* dsim, double* losses, float* losses32, void* ws, void* stream) {
    return pair_sum(sim, G, B, Bk, J, order, clip_offset, mask_mode, nullptr, dsim, losses, losses32, ws, stream);
}

extern "C" int facl_contrast_pair_sum(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                      float* dsim, double* losses, float* losses32, void* ws, void* stream) {
    return facl_contrast_pair_sum_mask(sim, G, B, Bk, J, order, clip_offset, MASK_ZERO, dsim, losses, losses32, ws, stream);
}

extern "C" int facl_loss_rows_fwd(const float* x, int64_t R, int C, int normalize, float s, float* n, float* inv_norm, void* stream) {
    if (!loss_rows_ok(R, C, normalize, s)) return FACL_E_SHAPE;
    if (!x || !n || !inv_norm) return FACL_E_NULL;
    if (((uintptr_t)x | (uintptr_t)n) & 15) return FACL_E_ALIGN;
    const dim3 grid((unsigned)((R + LR_WAVES - 1) / LR_WAVES));
    if (normalize) hipLaunchKernelGGL(k_loss_rows_fwd<true>, grid, dim3(LR_THREADS), 0, (hipStream_t)stream, x, (long long)R, C, s, n, inv_norm);
    else hipLaunchKernelGGL(k_loss_rows_fwd<false>, grid, dim3(LR_THREADS), 0, (hipStream_t)stream, x, (long long)R, C, s, n, inv_norm);
    return facl_launch_status();
}

extern "C" int facl_loss_rows_bwd(const float* dn, const float* n, const float* inv_norm, int64_t R, int C, int normalize, float s,
                                  float* dx, void* stream) {
    if (!loss_rows_ok(R, C, normalize, s)) return FACL_E_SHAPE;
    if (!dn || !n || !inv_norm || !dx) return FACL_E_NULL;
    if (((uintptr_t)dn | (uintptr_t)n | (uintptr_t)dx) & 15) return FACL_E_ALIGN;
    const dim3 grid((unsigned)((R + LR_WAVES - 1) / LR_WAVES));
    if (normalize) hipLaunchKernelGGL(k_loss_rows_bwd<true>, grid, dim3(LR_THREADS), 0, (hipStream_t)stream, dn, n, inv_norm, (long long)R, C, s, dx);
    else hipLaunchKernelGGL(k_loss_rows_bwd<false>, grid, dim3(LR_THREADS), 0, (hipStream_t)stream, dn, n, inv_norm, (long long)R, C, s, dx);
    return facl_launch_status();
}

extern "C" int facl_scale_rows2(const float* src, float* dst, int64_t R1, int64_t R, int J, const float* g1, const float* g2,
                                void* stream) {
    if (!src || !dst || !g1 || !g2) return FACL_E_NULL;
    if (R1 < 0 || R1 > R || R < 1 || J < 1) return FACL_E_SHAPE;
    const long long n = R * (long long)J, split = R1 * (long long)J;
    hipStream_t st = (hipStream_t)stream;
    if (!(n & 3) && !(split & 3) && !((((uintptr_t)src) | ((uintptr_t)dst)) & 15)) {
        const long long n4 = n / 4;
        hipLaunchKernelGGL((k_scale_rows2<float4>), dim3(grid_1d(n4)), dim3(256), 0, st, (const float4*)src, (float4*)dst, n4, split / 4, g1, g2);
    } else {
        hipLaunchKernelGGL((k_scale_rows2<float>), dim3(grid_1d(n)), dim3(256), 0, st, src, dst, n, split, g1, g2);
    }
    return facl_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
// The pair loss with a queue of negative keys from earlier steps.  sim_q ((G+1)*B, L) = [x ; x_global] @ queue^T holds, in its
// first `valid` columns (qstate = {head, valid}, read on the device: a captured step replays while the queue fills), extra
// negatives of every clip in both losses; they carry no clip identity, so MASK_ZERO and MASK_EXCLUDE do not touch them; under
// MASK_CLASS column k carries qcls[k], the class id of the clip that pushed it, and is masked iff the anchor's class is known
// and equal to it (q_load; a clip whose every column is masked has the partials (-inf, 0) everywhere, so M = -inf, S = 0 and
// lse = -inf: exactly 0 everywhere, as in the pair kernels).  Columns >= valid are
// never used (V = 4 loads the vector that straddles `valid` whole, inside the row, and q_load drops its dead lanes, NaN
// included) and their dsim_q is written as exactly 0.  A clip's block is now nA x (J + valid) values: too large for the
// register form, and 2B workgroups reading it three times would leave most CUs idle.  The block is therefore spread over
// workgroups by (row slot, chunk of QC columns) -- slots 0..G-2: circle anchors order[slot], slot G-1: the view that is no
// anchor (zero gradient row), slot G: the global loss's row; chunks: ceil(J / QC) of sim, then ceil(L / QC) of sim_q -- in
// two launches:
//   k_contrast_queue_part   per chunk (max, sum exp(v - max)) of the members of the log-sum-exp, the sum in fp64;
//   k_contrast_queue_write  every workgroup combines the partials of its clip's block in the same fixed order (the same lse
//                           bits in all of them, no atomic), evaluates the positives' terms and writes its chunk of dsim /
//                           dsim_q; the workgroup of (slot 0 | slot G, chunk 0) stores the clip's loss.
// MASK_SUP runs a third launch between the two, k_contrast_queue_pos (below): a clip's class cells are spread over the chunks and
// need lse, and the coefficient of the negatives needs their sums over all chunks.
// The chunk is held in registers inside each kernel (QC / QT values per thread); the same-clip column index advances by
// increments (one division per thread, see k_contrast_pair_reg).  V = 4: 16-byte loads and stores (J % 4 == L % 4 == 0).
namespace {
constexpr int QT = 256;                     // threads per workgroup
constexpr int QC = 2048;                    // columns per chunk
constexpr int QN = QC / QT;                 // values per thread

struct QUnit {
    PairSpec sp;
    int slot, ch, nch, c0, wlen, len;       // chunk: first column, columns written, leading columns that are live (queue: < valid)
    bool in_sim;                            // a chunk of sim (same-clip mask applies) or of sim_q
    size_t base;                            // element offset of the chunk in its matrix
};

__device__ __forceinline__ QUnit q_unit(int G, int B, int Bk, int J, int L, const long long* order, int clip_offset,
                                        const int* __restrict__ qstate) {
    const int cJ = (J + QC - 1) / QC, nch = cJ + (L + QC - 1) / QC;
    const int t = (int)(blockIdx.x / (unsigned)nch), slot = t % (G + 1);
    QUnit u{PairSpec(slot < G, t / (G + 1), G, B, Bk, J, clip_offset, order)};
    const PairSpec& sp = u.sp;
    u.slot = slot;
    u.nch = nch;
    u.ch = (int)(blockIdx.x % (unsigned)nch);
    const int v = qstate[1];
    const int valid = v < 0 ? 0 : (v > L ? L : v);         // clamped: a corrupt state cannot address outside sim_q / dsim_q
    const size_t r = (size_t)(u.slot == G ? G : sp.ord(u.slot)) * B + sp.n;
    u.in_sim = u.ch < cJ;
    if (u.in_sim) {
        u.c0 = u.ch * QC;
        u.wlen = J - u.c0 < QC ? J - u.c0 : QC;
        u.len = u.wlen;
        u.base = r * J + u.c0;
    } else {
        u.c0 = (u.ch - cJ) * QC;
        u.wlen = L - u.c0 < QC ? L - u.c0 : QC;
        const int live = valid - u.c0;
        u.len = live < 0 ? 0 : (live > u.wlen ? u.wlen : live);
        u.base = r * L + u.c0;
    }
    return u;
}

// The chunk's values into registers.  Bit i of `grad`: value i is a live column that is not a same-clip one (it receives a
// gradient); bit i of `mem`: it is a member of the log-sum-exp (MASK_ZERO: the same-clip columns too, as the value 0).
// MASK_CLASS: ids = cls (Bk) for a chunk of sim, looked up through the same-clip column index, or qcls (L) for a chunk of sim_q,
// read beside the values (V = 4: one 16-byte load, the launcher checks qcls's alignment); a queue column is masked iff the
// anchor's class is known and equals the column's.  Ids of dead lanes (columns >= valid) are never looked at.
// MASK_SUP: bit i of `*cell`: value i is a class cell (live, masked for its class and not for being the own clip); its value is
// kept in x[] although it is no member and has no bit in `grad`.
template <int MASK, int V>
__device__ __forceinline__ void q_load(const QUnit& u, const float* __restrict__ m, float (&x)[QN], unsigned& mem, unsigned& grad,
                                       const int* __restrict__ ids = nullptr, int mycls = -1, unsigned* cell = nullptr) {
    const float* src = m + u.base;
    const int Bk = u.sp.Bk;
    int jm = 0, step = 0;
    if (u.in_sim) { jm = (u.c0 + (int)threadIdx.x * V) % Bk; step = ((QT - 1) * V) % Bk; }
    mem = grad = 0u;
#pragma unroll
    for (int k = 0; k < QN / V; ++k) {
        const int e = (k * QT + (int)threadIdx.x) * V;
        float v[V];
        int id[V];
#pragma unroll
        for (int c = 0; c < V; ++c) { v[c] = 0.f; id[c] = -1; }
        if (e < u.len) {                                   // V = 4: wlen % 4 == 0, the whole vector lies inside the row
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(src + e);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = src[e];
            }
            if constexpr (MASK >= MASK_CLASS) {
                if (!u.in_sim && mycls >= 0) {             // workgroup-uniform
                    if constexpr (V == 4) {
                        const int4 q = *reinterpret_cast<const int4*>(ids + u.c0 + e);
                        id[0] = q.x; id[1] = q.y; id[2] = q.z; id[3] = q.w;
                    } else {
                        id[0] = ids[u.c0 + e];
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const bool live = e + c < u.len;
            bool masked = u.in_sim && jm == u.sp.myclip;
            if constexpr (MASK >= MASK_CLASS) {
                if (u.in_sim) masked = live && col_masked<MASK>(jm, u.sp.myclip, mycls, ids);
                else masked = mycls >= 0 && id[c] == mycls;
            }
            const bool g = live && !masked;
            bool keep = g;
            if constexpr (MASK == MASK_SUP) {
                const bool cc = live && masked && !(u.in_sim && jm == u.sp.myclip);
                *cell |= (unsigned)cc << (k * V + c);
                keep = g || cc;
            }
            x[k * V + c] = keep ? v[c] : 0.f;
            grad |= (unsigned)g << (k * V + c);
            mem |= (unsigned)(MASK == MASK_ZERO ? live : g) << (k * V + c);
            if (u.in_sim && ++jm == Bk) jm = 0;
        }
        if (u.in_sim) { jm += step; if (jm >= Bk) jm -= Bk; }
    }
}

template <int MASK, int V>
__global__ __launch_bounds__(QT) void k_contrast_queue_part(const float* __restrict__ sim, const float* __restrict__ sim_q, int G,
                                                            int B, int Bk, int J, int L, const long long* __restrict__ order,
                                                            int clip_offset, const int* __restrict__ qstate,
                                                            float* __restrict__ pm, double* __restrict__ ps,
                                                            const int* __restrict__ cls, const int* __restrict__ qcls,
                                                            int* __restrict__ pc) {
    __shared__ float smf[QT / 64];
    __shared__ double smd[QT / 64];
    const QUnit u = q_unit(G, B, Bk, J, L, order, clip_offset, qstate);
    if (u.slot == G - 1) return;                           // no anchor: no member of any log-sum-exp
    float x[QN];
    unsigned mem, grad, cell = 0u;
    if constexpr (MASK >= MASK_CLASS) q_load<MASK, V>(u, u.in_sim ? sim : sim_q, x, mem, grad, u.in_sim ? cls : qcls, cls[u.sp.myclip], &cell);
    else q_load<MASK, V>(u, u.in_sim ? sim : sim_q, x, mem, grad);
    float mx = -INFINITY;                                  // a chunk without a member: (-inf, 0), skipped by the combination
#pragma unroll
    for (int i = 0; i < QN; ++i)
        if ((mem >> i) & 1u) mx = fmaxf(mx, x[i]);
    mx = block_reduce_max(mx, smf);
    double se = 0;
#pragma unroll
    for (int i = 0; i < QN; ++i)
        if ((mem >> i) & 1u) se += (double)__expf(x[i] - mx);
    se = block_reduce_sum(se, smd);
    if (threadIdx.x == 0) { pm[blockIdx.x] = mx; ps[blockIdx.x] = se; }
    if constexpr (MASK == MASK_SUP) {                      // the chunk's class cells, counted
        const int cn = block_reduce_count(__popc(cell), reinterpret_cast<int*>(smf));
        if (threadIdx.x == 0) pc[blockIdx.x] = cn;
    }
}

// The log-sum-exp of a clip's block from its nA * nch chunk partials, which start at p0 (circle: slots 0..G-2 are adjacent
// units): every workgroup of the block combines them in the same fixed order -- the same lse bits in all of them, no atomic.
__device__ __forceinline__ float q_lse(const float* __restrict__ pm, const double* __restrict__ ps, size_t p0, int np, float* smf,
                                       double* smd) {
    float M = -INFINITY;
    for (int p = threadIdx.x; p < np; p += QT)
        if (ps[p0 + p] != 0) M = fmaxf(M, pm[p0 + p]);     // != 0, not > 0: a NaN partial (a NaN / inf similarity) is no empty chunk
    M = block_reduce_max(M, smf);
    double S = 0;
    for (int p = threadIdx.x; p < np; p += QT) {
        const double s = ps[p0 + p];
        if (s != 0) S += s * exp((double)pm[p0 + p] - (double)M);
    }
    S = block_reduce_sum(S, smd);
    return M + (float)log(S);
}

// MASK_SUP only, between the two launches above, on the same grid and units: lse as the write kernel forms it, then the chunk's
// class cells as positive slots against it; per chunk (sum of terms, sum of dlse shares) in fp64 into pt / pd.
template <int V>
__global__ __launch_bounds__(QT) void k_contrast_queue_pos(const float* __restrict__ sim, const float* __restrict__ sim_q, int G,
                                                           int B, int Bk, int J, int L, const long long* __restrict__ order,
                                                           int clip_offset, const int* __restrict__ qstate,
                                                           const float* __restrict__ pm, const double* __restrict__ ps,
                                                           const int* __restrict__ cls, const int* __restrict__ qcls,
                                                           const int* __restrict__ pc, double* __restrict__ pt,
                                                           double* __restrict__ pd) {
    __shared__ float smf[QT / 64];
    __shared__ double smd[QT / 64];
    const QUnit u = q_unit(G, B, Bk, J, L, order, clip_offset, qstate);
    const PairSpec& sp = u.sp;
    if (u.slot == G - 1) return;                           // no anchor
    if (pc[blockIdx.x] == 0) return;                       // workgroup-uniform; the write kernel reads no sums of such a chunk
    float x[QN];
    unsigned mem, grad, cell = 0u;
    q_load<MASK_SUP, V>(u, u.in_sim ? sim : sim_q, x, mem, grad, u.in_sim ? cls : qcls, cls[sp.myclip], &cell);
    const float lse = q_lse(pm, ps, ((size_t)sp.n * (G + 1) + (sp.circle ? 0 : G)) * u.nch, sp.nA * u.nch, smf, smd);
    double ct = 0, cd = 0;
#pragma unroll
    for (int i = 0; i < QN; ++i)
        if ((cell >> i) & 1u) {
            const SlotTerm st = slot_term(x[i], lse);
            ct += (double)st.loss;
            cd += (double)st.dlse;
        }
    ct = block_reduce_sum(ct, smd);
    cd = block_reduce_sum(cd, smd);
    if (threadIdx.x == 0) { pt[blockIdx.x] = ct; pd[blockIdx.x] = cd; }
}

template <int MASK, int V>
__global__ __launch_bounds__(QT) void k_contrast_queue_write(const float* __restrict__ sim, const float* __restrict__ sim_q, int G,
                                                             int B, int Bk, int J, int L, const long long* __restrict__ order,
                                                             int clip_offset, const int* __restrict__ qstate,
                                                             const float* __restrict__ pm, const double* __restrict__ ps,
                                                             float* __restrict__ dsim, float* __restrict__ dsim_q,
                                                             double* __restrict__ part, const int* __restrict__ cls,
                                                             const int* __restrict__ qcls, const int* __restrict__ pc,
                                                             const double* __restrict__ pt, const double* __restrict__ pd,
                                                             float pw) {
    __shared__ float smf[QT / 64];
    __shared__ double smd[QT / 64];
    const QUnit u = q_unit(G, B, Bk, J, L, order, clip_offset, qstate);
    const PairSpec& sp = u.sp;
    float* dst = (u.in_sim ? dsim : dsim_q) + u.base;
    float x[QN];
    unsigned mem = 0u, grad = 0u, cell = 0u;
    float lse = 0.f, dlse = 0.f, wB = 0.f;                 // wB (MASK_SUP): w / B, the factor on a class cell's dpos
    double loss = 0;
    const float invB = 1.f / (float)B;
    if (u.slot != G - 1) {                                 // workgroup-uniform
        // requested ahead of the reductions below
        if constexpr (MASK >= MASK_CLASS) q_load<MASK, V>(u, u.in_sim ? sim : sim_q, x, mem, grad, u.in_sim ? cls : qcls, cls[sp.myclip], &cell);
        else q_load<MASK, V>(u, u.in_sim ? sim : sim_q, x, mem, grad);
        const int np = sp.nA * u.nch;
        const size_t p0 = ((size_t)sp.n * (G + 1) + (sp.circle ? 0 : G)) * u.nch;
        lse = q_lse(pm, ps, p0, np, smf, smd);
        double loss_t = 0, dlse_t = 0;
        for (int s = threadIdx.x; s < sp.nS; s += QT) {
            const SlotTerm st = slot_term(sim[sp.pos_index(s)], lse);
            loss_t += (double)st.loss;
            dlse_t += (double)st.dlse;
        }
        loss = block_reduce_sum(loss_t, smd);
        const double dlse_s = block_reduce_sum(dlse_t, smd);
        dlse = (float)dlse_s * invB;
        if constexpr (MASK == MASK_SUP) {                  // the block's class cells from their chunk partials, the same fixed order
            int cn = 0;
            double ct = 0, cd = 0;
            for (int p = threadIdx.x; p < np; p += QT) {
                const int c = pc[p0 + p];
                if (c > 0) { cn += c; ct += pt[p0 + p]; cd += pd[p0 + p]; }
            }
            cn = block_reduce_count(cn, reinterpret_cast<int*>(smf));
            if (cn > 0) {                                  // workgroup-uniform
                const double w = sup_weight(pw, sp.nS, cn);
                loss += w * block_reduce_sum(ct, smd);
                dlse = (float)(dlse_s + w * block_reduce_sum(cd, smd)) * invB;
                wB = (float)w * invB;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < QN / V; ++k) {
        const int e = (k * QT + (int)threadIdx.x) * V;
        if (e < u.wlen) {
            float d[V];
#pragma unroll
            for (int c = 0; c < V; ++c) {
                d[c] = ((grad >> (k * V + c)) & 1u) ? dlse * __expf(x[k * V + c] - lse) : 0.f;
                if constexpr (MASK == MASK_SUP)
                    if ((cell >> (k * V + c)) & 1u) d[c] = wB * slot_term(x[k * V + c], lse).dpos;
            }
            if constexpr (V == 4) *reinterpret_cast<float4*>(dst + e) = make_float4(d[0], d[1], d[2], d[3]);
            else dst[e] = d[0];
        }
    }
    if (u.slot == G - 1 || !u.in_sim) return;
    __syncthreads();                                       // the positives overwrite zeros written just above
    // positives that lie in this chunk: the circle slot's own one, every view's for the global row
    for (int s = threadIdx.x; s < sp.nS; s += QT) {
        if (sp.circle && s != u.slot) continue;
        const int col = (sp.circle ? sp.ord(s + 1) : s) * Bk + sp.myclip;
        if (col < u.c0 || col >= u.c0 + u.wlen) continue;
        const size_t pp = sp.pos_index(s);
        dsim[pp] = slot_term(sim[pp], lse).dpos * invB;
    }
    if (u.ch == 0 && (u.slot == 0 || u.slot == G) && threadIdx.x == 0) part[2 * sp.n + sp.circle] = loss * (double)invB;
}

// head clamped to a multiple of P below L: a corrupt state cannot address outside the queue
__device__ __forceinline__ int q_head(const int* qstate, int P, int L) {
    int h = qstate[0];
    if (h < 0) h = 0;
    h -= h % P;
    return h > L - P ? L - P : h;
}

__global__ __launch_bounds__(256) void k_queue_push(const float4* __restrict__ rows, long long n4, int P, int C4,
                                                    float4* __restrict__ queue, int L, const int* __restrict__ qstate) {
    float4* dst = queue + (size_t)q_head(qstate, P, L) * C4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) dst[i] = rows[i];
}

// its own launch, behind the copy in stream order: no workgroup of the copy reads `head` after it has moved
__global__ __launch_bounds__(64) void k_queue_advance(int* __restrict__ qstate, int P, int L) {
    if (threadIdx.x == 0) {
        const int h = q_head(qstate, P, L), v = qstate[1];
        const int valid = v < 0 ? 0 : (v > L ? L : v);
        qstate[0] = (h + P) % L;
        qstate[1] = valid + P > L ? L : valid + P;
    }
}

// cls / qcls: the class ids of MASK_CLASS / MASK_SUP; the entry with a mask_mode argument passes none, and modes 2 and 3 are no
// modes of its.  pw: MASK_SUP's weight.
int pair_queue(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L, const int64_t* order, int clip_offset,
               int mask_mode, const int32_t* cls, const int32_t* qcls, const int32_t* qstate, float* dsim, float* dsim_q,
               double* losses, float* losses32, void* ws, void* stream, float pw = 0.f) {
    if (!sim || !sim_q || !order || !qstate || !dsim || !dsim_q || !losses || !losses32 || !ws) return FACL_E_NULL;
    // Bk >= 2 outside `zero` here too: the queue may be empty
    if (!pair_shape_ok(G, B, Bk, J, clip_offset, mask_mode, cls && qcls) || L < 1) return FACL_E_SHAPE;
    if (J > 0x7fffffff - QC || L > 0x7fffffff - QC) return FACL_E_SHAPE;      // the kernels round both up to chunks in int
    const long long nch = (J + QC - 1) / QC + (L + QC - 1) / QC, units = (long long)(G + 1) * B * nch;
    if (units > 0x7fffffffLL) return FACL_E_SHAPE;
    // workspace: [per-clip losses (2B doubles) | chunk sums (units doubles) | chunk maxima (units floats)]; MASK_SUP: the
    // doubles grow by the chunks' class-cell terms and dlse shares (units each), and the cell counts (units ints) follow the maxima
    const size_t nd = mask_mode == MASK_SUP ? 3 : 1, ni = mask_mode == MASK_SUP ? 1 : 0;
    if ((size_t)(2 * (long long)B + nd * units) * sizeof(double) + (size_t)units * (sizeof(float) + ni * sizeof(int)) >
        (size_t)facl_ws_bytes()) return FACL_E_SHAPE;
    double* part = (double*)ws;
    double* ps = part + 2 * (size_t)B;
    double* pt = ps + units;                               // MASK_SUP only, as pd and pc
    double* pd = pt + units;
    float* pm = (float*)(ps + nd * units);
    int* pc = (int*)(pm + units);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = J % 4 == 0 && L % 4 == 0 && !(((uintptr_t)sim | (uintptr_t)sim_q | (uintptr_t)dsim | (uintptr_t)dsim_q) & 15);
    with_mask(mask_mode, [&](auto m) {
        constexpr int MASK = decltype(m)::value;
        auto launch = [&](auto v) {
            constexpr int V = decltype(v)::value;
            hipLaunchKernelGGL((k_contrast_queue_part<MASK, V>), dim3((unsigned)units), dim3(QT), 0, st, sim, sim_q, G, B, Bk, J, L,
                               (const long long*)order, clip_offset, (const int*)qstate, pm, ps, (const int*)cls, (const int*)qcls, pc);
            if constexpr (MASK == MASK_SUP)
                hipLaunchKernelGGL((k_contrast_queue_pos<V>), dim3((unsigned)units), dim3(QT), 0, st, sim, sim_q, G, B, Bk, J, L,
                                   (const long long*)order, clip_offset, (const int*)qstate, (const float*)pm, (const double*)ps,
                                   (const int*)cls, (const int*)qcls, (const int*)pc, pt, pd);
            hipLaunchKernelGGL((k_contrast_queue_write<MASK, V>), dim3((unsigned)units), dim3(QT), 0, st, sim, sim_q, G, B, Bk, J, L,
                               (const long long*)order, clip_offset, (const int*)qstate, (const float*)pm, (const double*)ps, dsim,
                               dsim_q, part, (const int*)cls, (const int*)qcls, (const int*)pc, (const double*)pt, (const double*)pd, pw);
        };
        // MASK_CLASS / MASK_SUP read qcls beside the values: 16-byte loads need it aligned too
        if (vec && (MASK < MASK_CLASS || !((uintptr_t)qcls & 15))) launch(std::integral_constant<int, 4>{});
        else launch(std::integral_constant<int, 1>{});
    });
    int rc = facl_launch_status();
    return rc ? rc : finish_losses(part, B, losses, losses32, st);
}

// slots [head, head + P) of the ids beside the queue's rows; `head` as k_queue_push reads it (this launch runs BEFORE
// facl_queue_push's advance in stream order) and the state is left as it is
__global__ __launch_bounds__(256) void k_queue_push_ids(const int* __restrict__ ids, int P, int* __restrict__ qcls, int L,
                                                        const int* __restrict__ qstate) {
    int* dst = qcls + q_head(qstate, P, L);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) dst[i] = ids[i];
}
}  // namespace

extern "C" int facl_contrast_pair_queue(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L,
                                        const int64_t* order, int clip_offset, int mask_mode, const int32_t* qstate, float* dsim,
                                        float* dsim_q, double* losses, float* losses32, void* ws, void* stream) {
    return pair_queue(sim, sim_q, G, B, Bk, J, L, order, clip_offset, mask_mode, nullptr, nullptr, qstate, dsim, dsim_q, losses,
                      losses32, ws, stream);
}

// the pair loss and its queue form under the class-aware mask (MASK_CLASS above)
extern "C" int facl_contrast_pair_sum_cls(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                          const int32_t* cls, float* dsim, double* losses, float* losses32, void* ws, void* stream) {
    if (!cls) return FACL_E_NULL;
    return pair_sum(sim, G, B, Bk, J, order, clip_offset, MASK_CLASS, cls, dsim, losses, losses32, ws, stream);
}

extern "C" int facl_contrast_pair_queue_cls(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L,
                                            const int64_t* order, int clip_offset, const int32_t* cls, const int32_t* qcls,
                                            const int32_t* qstate, float* dsim, float* dsim_q, double* losses, float* losses32,
                                            void* ws, void* stream) {
    if (!cls || !qcls) return FACL_E_NULL;
    return pair_queue(sim, sim_q, G, B, Bk, J, L, order, clip_offset, MASK_CLASS, cls, qcls, qstate, dsim, dsim_q, losses, losses32,
                      ws, stream);
}

// class-mates as extra positives (MASK_SUP above), weight pos_weight
extern "C" int facl_contrast_pair_sum_sup(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                          const int32_t* cls, float pos_weight, float* dsim, double* losses, float* losses32,
                                          void* ws, void* stream) {
    if (!cls) return FACL_E_NULL;
    if (!pos_weight_ok(pos_weight)) return FACL_E_SHAPE;
    return pair_sum(sim, G, B, Bk, J, order, clip_offset, MASK_SUP, cls, dsim, losses, losses32, ws, stream, pos_weight);
}

extern "C" int facl_contrast_pair_queue_sup(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L,
                                            const int64_t* order, int clip_offset, const int32_t* cls, const int32_t* qcls,
                                            const int32_t* qstate, float pos_weight, float* dsim, float* dsim_q, double* losses,
                                            float* losses32, void* ws, void* stream) {
    if (!cls || !qcls) return FACL_E_NULL;
    if (!pos_weight_ok(pos_weight)) return FACL_E_SHAPE;
    return pair_queue(sim, sim_q, G, B, Bk, J, L, order, clip_offset, MASK_SUP, cls, qcls, qstate, dsim, dsim_q, losses, losses32,
                      ws, stream, pos_weight);
}

extern "C" int facl_queue_push_ids(const int32_t* ids, int P, int32_t* qcls, int L, const int32_t* qstate, void* stream) {
    if (P < 1 || L < 1 || L % P) return FACL_E_SHAPE;
    if (!ids || !qcls || !qstate) return FACL_E_NULL;
    hipLaunchKernelGGL(k_queue_push_ids, dim3(grid_1d(P)), dim3(256), 0, (hipStream_t)stream, (const int*)ids, P, (int*)qcls, L,
                       (const int*)qstate);
    return facl_launch_status();
}

extern "C" int facl_queue_push(const float* rows, int P, int C, float* queue, int L, int32_t* qstate, void* stream) {
    if (P < 1 || C < 4 || C % 4 || L < 1 || L % P) return FACL_E_SHAPE;
    if (!rows || !queue || !qstate) return FACL_E_NULL;
    if (((uintptr_t)rows | (uintptr_t)queue) & 15) return FACL_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const long long n4 = (long long)P * (C / 4);
    hipLaunchKernelGGL(k_queue_push, dim3(grid_1d(n4)), dim3(256), 0, st, (const float4*)rows, n4, P, C / 4, (float4*)queue, L,
                       (const int*)qstate);
    hipLaunchKernelGGL(k_queue_advance, dim3(1), dim3(64), 0, st, (int*)qstate, P, L);
    return facl_launch_status();
}
