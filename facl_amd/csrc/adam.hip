// The "all tensors in one launch" kernels of the step: Adam (cn3d_train_motion_GL.py:180,:332: torch.optim.Adam(lr 3e-4,
// betas (0.5, 0.999), eps 1e-6), no weight decay, no amsgrad), the momentum average of the key encoder that follows it
// (facl_amd/key_encoder.py; MoCo's _momentum_update_key_encoder, parameters only) and the optimizer recipe of the contrastive
// modes (facl_amd/optim.py: weight_decay, max_grad_norm, schedule; off by default -- the first three entries are then
// the whole step).  torch's fused multi-tensor kernel walks 64 K-element chunks: 2.36 M parameters are 36 workgroups (47 us on
// 256 CUs); here a workgroup takes FACL_ADAM_CHUNK = 2048 elements (~1150 workgroups, HBM-bound: 7 x 9.4 MB per Adam step).
// What the chunked kernels share is stated once:
//   ChunkTable<NP>  NP columns of tensor pointers, the element counts and the first chunk of every tensor, BY VALUE in the kernel
//                   arguments (no device-side table to keep coherent; a HIP graph bakes the pointers at capture time, when the
//                   gradient buffers of the captured step are fixed); chunk_table() checks the caller's host arrays and fills it
//   chunk_of()      blockIdx.x -> (tensor, its first chunk, its element count)
//   chunk_walk()    the chunk's elements: two float4 per thread where every column allows it (every tensor of the model does),
//                   all loads before the first store, else eight scalar elements
//   adam_update()   the Adam update of one element, plain or with the recipe's clip coefficient and decay
// The entries:
//   facl_adam_prep: step += 1; consts = (lr / (1 - b1^t), 1 / sqrt(1 - b2^t))      -- one thread, device-resident lr / step
//   facl_adam_apply: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
//   facl_ema_apply: pk = m pk + (1-m) p
//   facl_grad_sqnorm: partial[chunk] = sum of g^2 over the chunk in fp64, fixed order, no atomics  -- only when clipping
//   facl_adam_prep_ex: step += 1; norm = sqrt(sum of the partials), c = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_);
//                      lr_t = warm-up x (host lr | cosine) from the step counter; consts = (lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t),
//                      lr_t, c, norm)
//   facl_adamw_apply: g' = c g; p *= 1 - lr_t wd on flagged tensors (torch.optim.AdamW's order); then facl_adam_apply's update on g'
// SGD with momentum and LARS (facl_amd/optim.py: FusedSGD) are a second update rule on the same table, walk, sums
// and device-side step / rate / clip / schedule:
//   facl_tensor_sqnorms: facl_grad_sqnorm on two columns in one pass, partial_p[chunk] = sum p^2, partial_g[chunk] = sum g^2  -- LARS
//   facl_sgd_prep: step += 1; lr_t, c, norm as facl_adam_prep_ex; consts = (lr_t, 0, lr_t, c, norm); under LARS the trust ratio of
//                  every tensor from the partials of its own chunks: eta |p| / (c |g| + wd |p|) on the flagged tensors, else 1
//   facl_sgd_apply: d = (c g + wd p on flagged tensors) * trust; buf = mu buf + d; p -= lr_t (buf | d + mu buf under Nesterov)
#include "common.h"
#include <math.h>
#include <stdint.h>

template <int NP>
struct ChunkTable {
    float* col[NP][FACL_ADAM_MAX_TENSORS];
    int n[FACL_ADAM_MAX_TENSORS];
    int chunk0[FACL_ADAM_MAX_TENSORS + 1];        // first chunk of tensor i (prefix sums of ceil(n / CHUNK))
    int nt;
};

struct AdamWTable {
    ChunkTable<4> t;
    unsigned char decay[FACL_ADAM_MAX_TENSORS];   // 1: the tensor is weight-decayed
};

struct SgdTable {
    ChunkTable<3> t;
    unsigned char mask[FACL_ADAM_MAX_TENSORS];    // 1: the tensor is weight-decayed and, under LARS, adapted
};

struct SgdPrefix {                                // what facl_sgd_prep needs of the chunk table, BY VALUE like the table itself
    int chunk0[FACL_ADAM_MAX_TENSORS + 1];
    unsigned char mask[FACL_ADAM_MAX_TENSORS];
    int nt;                                       // 0: plain SGD, no trust ratio is formed
};

namespace {

// cols: NP HOST arrays of nt device pointers; n: HOST array of element counts.  Returns the number of chunks (the grid), or
// FACL_E_NULL for a NULL array or entry, FACL_E_SHAPE for nt outside 1..FACL_ADAM_MAX_TENSORS or an n[i] < 1.
template <int NP>
int chunk_table(ChunkTable<NP>& tb, int nt, const float* const* const (&cols)[NP], const int* n) {
    for (int c = 0; c < NP; ++c)
        if (!cols[c]) return FACL_E_NULL;
    if (!n) return FACL_E_NULL;
    if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
    int chunks = 0;
    for (int i = 0; i < nt; ++i) {
        for (int c = 0; c < NP; ++c) {
            if (!cols[c][i]) return FACL_E_NULL;
            tb.col[c][i] = const_cast<float*>(cols[c][i]);
        }
        if (n[i] < 1) return FACL_E_SHAPE;
        tb.n[i] = n[i];
        tb.chunk0[i] = chunks;
        chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
    }
    tb.chunk0[nt] = chunks;
    tb.nt = nt;
    return chunks;
}

struct Chunk { int t, first, n; };                // tensor, its first chunk, its elements

// tensor of this workgroup's chunk: binary search in the prefix table (wave-uniform)
template <int NP>
__device__ __forceinline__ Chunk chunk_of(const ChunkTable<NP>& tb) {
    int lo = 0, hi = tb.nt;
    const int c = blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    return {lo, tb.chunk0[lo], tb.n[lo]};
}

// f(x, E) on the chunk's elements: x[c][0..E) holds E consecutive elements of column c, and the columns whose bit is set in WR
// are stored back afterwards.  E = 4, 16 bytes per lane, where the tensor allows it: a quarter of the memory instructions of the
// scalar walk (E = 1), all of a thread's loads in flight before its first store.  Nothing outside [0, n) is touched.
template <unsigned WR, int NC, class F>
__device__ __forceinline__ void chunk_walk(float* const (&col)[NC], const Chunk ck, F f) {
    const int base = ((int)blockIdx.x - ck.first) * FACL_ADAM_CHUNK;
    uintptr_t bits = ck.n & 3;
#pragma unroll
    for (int c = 0; c < NC; ++c) bits |= (uintptr_t)col[c];
    if (!(bits & 15)) {
        float4 x4[2][NC];
        int i4[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            i4[k] = (base >> 2) + k * 256 + threadIdx.x;
            if (4 * i4[k] < ck.n) {
#pragma unroll
                for (int c = 0; c < NC; ++c) x4[k][c] = reinterpret_cast<const float4*>(col[c])[i4[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (4 * i4[k] >= ck.n) continue;
            float x[NC][4];
#pragma unroll
            for (int c = 0; c < NC; ++c) { x[c][0] = x4[k][c].x; x[c][1] = x4[k][c].y; x[c][2] = x4[k][c].z; x[c][3] = x4[k][c].w; }
            f(x, 4);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (WR >> c & 1) reinterpret_cast<float4*>(col[c])[i4[k]] = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < FACL_ADAM_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < ck.n) {
            float x[NC][4];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c][0] = col[c][i];
            f(x, 1);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (WR >> c & 1) col[c][i] = x[c][0];
        }
    }
}

// t = step + 1, stored; the two bias corrections of step t in fp64
__device__ __forceinline__ float adam_advance(float* __restrict__ step, float b1, float b2, double& bc1, double& bc2) {
    const float t = step[0] + 1.f;
    step[0] = t;
    bc1 = 1.0 - pow((double)b1, (double)t);
    bc2 = 1.0 - pow((double)b2, (double)t);
    return t;
}

__global__ void k_adam_prep(const float* __restrict__ lr, float* __restrict__ step, float b1, float b2,
                            float* __restrict__ consts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double bc1, bc2;
    adam_advance(step, b1, b2, bc1, bc2);
    consts[0] = (float)((double)lr[0] / bc1);
    consts[1] = (float)(1.0 / sqrt(bc2));
}

struct AdamCoef { float b1, om1, b2, om2, eps, step_size, isb2, clip, keep; };      // om = 1 - b; clip, keep: the recipe's form only

// The update of one element.  RECIPE: the clip coefficient on the gradient VALUE (p.grad is only read) and the decoupled decay in
// front of the update, torch.optim.AdamW's param.mul_(1 - lr * weight_decay).  With clip == 1.0f and keep == 1.0f both products
// are x * 1.0f, which is exact, and everything else is the one expression below (the build has -ffp-contract=off): the two forms
// give the same bits.
template <bool RECIPE>
__device__ __forceinline__ void adam_update(const AdamCoef& k, float& p, float g, float& m, float& v) {
    if (RECIPE) { g = g * k.clip; p = p * k.keep; }
    m = k.b1 * m + k.om1 * g;
    v = k.b2 * v + k.om2 * g * g;
    p -= k.step_size * (m / (sqrtf(v) * k.isb2 + k.eps));
}

template <bool RECIPE>
__device__ __forceinline__ void adam_chunk(const ChunkTable<4>& tb, const Chunk ck, const AdamCoef k) {
    // the table's columns are p, g, m, v; walked g, m, v, p, the order in which the loads are issued
    float* const col[4] = {tb.col[1][ck.t], tb.col[2][ck.t], tb.col[3][ck.t], tb.col[0][ck.t]};
    chunk_walk<0b1110>(col, ck, [&](float (&x)[4][4], int E) {
        for (int e = 0; e < E; ++e) adam_update<RECIPE>(k, x[3][e], x[0][e], x[1][e], x[2][e]);
    });
}

__global__ __launch_bounds__(256) void k_adam_apply(ChunkTable<4> tb, const float* __restrict__ consts, float b1, float b2,
                                                    float eps) {
    const AdamCoef k = {b1, 1.f - b1, b2, 1.f - b2, eps, consts[0], consts[1], 1.f, 1.f};     // read while the search runs
    adam_chunk<false>(tb, chunk_of(tb), k);
}

__global__ __launch_bounds__(256) void k_adamw_apply(AdamWTable tw, const float* __restrict__ consts, float b1, float b2,
                                                     float eps, float wd) {
    const Chunk ck = chunk_of(tw.t);
    const float keep = tw.decay[ck.t] ? 1.f - consts[2] * wd : 1.f;
    adam_chunk<true>(tw.t, ck, {b1, 1.f - b1, b2, 1.f - b2, eps, consts[0], consts[1], consts[3], keep});
}

// pk = m pk + (1-m) p.  Three roundings and the one of 1 - m (the build has -ffp-contract=off); m = 0 copies p and m = 1 leaves pk
// as it is through the formula itself: 0 * finite = 0, x + 0 = x.
__global__ __launch_bounds__(256) void k_ema_apply(ChunkTable<2> tb, float m) {
    const Chunk ck = chunk_of(tb);
    float* const col[2] = {tb.col[0][ck.t], tb.col[1][ck.t]};                     // pk, p
    const float om = 1.f - m;
    chunk_walk<0b01>(col, ck, [&](float (&x)[2][4], int E) {
        for (int e = 0; e < E; ++e) x[0][e] = m * x[0][e] + om * x[1][e];
    });
}

// Sum over the 256 threads of a workgroup in one fixed order: the xor butterfly inside each wave (every lane ends with the same
// bits), then the four wave sums through LDS, added 0, 1, 2, 3.  Valid in thread 0.
__device__ __forceinline__ double wg256_sum_f64(double s, double* red) {
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// partial[chunk] = sum of g^2 over the chunk.  Every element is widened to fp64 first: the square of an fp32 value has 48
// significant bits and is exact in fp64, so the only roundings are those of the additions, whose order is fixed by (chunk, thread):
// the squares of a float4 left to right, then onto the thread's sum.
__global__ __launch_bounds__(256) void k_grad_sqnorm(ChunkTable<1> tb, double* __restrict__ partial) {
    __shared__ double red[4];
    const Chunk ck = chunk_of(tb);
    float* const col[1] = {tb.col[0][ck.t]};
    double s = 0.0;
    chunk_walk<0>(col, ck, [&](float (&x)[1][4], int E) {
        double q = (double)x[0][0] * (double)x[0][0];
        for (int e = 1; e < E; ++e) q += (double)x[0][e] * (double)x[0][e];
        s += q;
    });
    s = wg256_sum_f64(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The learning rate of step tt (1-based) in fp64: the warm-up factor min(1, tt / W) times the host's rate lr0 or the half cosine
// from lr0 at tt = W down to lr_min at tt = T.  The one evaluation of both preps (facl_amd.optim.lr_at_step is its host form).
__device__ __forceinline__ double scheduled_lr(double lr0, double tt, int cosine, int W, int T, double lr_min) {
    const double warm = W > 0 ? fmin(1.0, tt / (double)W) : 1.0;
    double lr_s = lr0;
    if (cosine) {
        const double tp = fmax(tt - (double)W, 0.0), Tp = (double)(T - W);
        lr_s = lr_min + (lr0 - lr_min) * 0.5 * (1.0 + cos(M_PI * fmin(tp, Tp) / Tp));
    }
    return warm * lr_s;
}

// One workgroup of 256 threads.  consts = (lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t), lr_t, c, norm); np == 0: no clipping, c = 1 exactly.
// A non-finite norm goes the way it goes in torch.nn.utils.clip_grad_norm_: inf gives c = 0 (and 0 * inf = NaN in the update),
// NaN gives c = NaN (the comparison of the clamp is false).
__global__ __launch_bounds__(256) void k_adam_prep_ex(const float* __restrict__ lr, float* __restrict__ step, float b1, float b2,
                                                      const double* __restrict__ partial, int np, double max_norm, int cosine,
                                                      int W, int T, double lr_min, float* __restrict__ consts) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
    s = wg256_sum_f64(s, red);
    if (threadIdx.x != 0) return;
    double bc1, bc2;
    const double tt = (double)adam_advance(step, b1, b2, bc1, bc2);
    const double lr_t = scheduled_lr((double)lr[0], tt, cosine, W, T, lr_min);
    double norm = 0.0, c = 1.0;
    if (np > 0) {
        norm = sqrt(s);
        c = max_norm / (norm + 1e-6);
        if (c > 1.0) c = 1.0;
    }
    consts[0] = (float)(lr_t / bc1);
    consts[1] = (float)(1.0 / sqrt(bc2));
    consts[2] = (float)lr_t;
    consts[3] = (float)c;
    consts[4] = (float)norm;
}

// k_grad_sqnorm on two columns in one pass: partial_p[chunk] = sum of p^2, partial_g[chunk] = sum of g^2, each with k_grad_sqnorm's
// own additions in its own order, so partial_g holds the bits that kernel writes.  The walk issues the two float4 of both
// columns, four 16-byte loads per thread, before the first square.
__global__ __launch_bounds__(256) void k_tensor_sqnorms(ChunkTable<2> tb, double* __restrict__ partial_p,
                                                        double* __restrict__ partial_g) {
    __shared__ double red[2][4];
    const Chunk ck = chunk_of(tb);
    float* const col[2] = {tb.col[0][ck.t], tb.col[1][ck.t]};                     // p, g
    double sp = 0.0, sg = 0.0;
    chunk_walk<0>(col, ck, [&](float (&x)[2][4], int E) {
        double qp = (double)x[0][0] * (double)x[0][0], qg = (double)x[1][0] * (double)x[1][0];
        for (int e = 1; e < E; ++e) {
            qp += (double)x[0][e] * (double)x[0][e];
            qg += (double)x[1][e] * (double)x[1][e];
        }
        sp += qp;
        sg += qg;
    });
    sp = wg256_sum_f64(sp, red[0]);
    sg = wg256_sum_f64(sg, red[1]);
    if (threadIdx.x == 0) {
        partial_p[blockIdx.x] = sp;
        partial_g[blockIdx.x] = sg;
    }
}

// One workgroup of 256 threads.  consts = (lr_t, 0, lr_t, c, norm): slots 2..4 as k_adam_prep_ex writes them, by the same
// operations in the same order (the sum of the partials included).  px.nt > 0 (LARS): wave w takes the tensors w, w + 4, ...;
// its lanes add the tensor's partials lane-strided, then the butterfly: one fixed order.  The clip coefficient enters |g| as
// the fp32 value that k_sgd_apply multiplies the gradient by.
__global__ __launch_bounds__(256) void k_sgd_prep(const float* __restrict__ lr, float* __restrict__ step,
                                                  const double* __restrict__ partial_g, const double* __restrict__ partial_p,
                                                  int np, SgdPrefix px, double max_norm, int clip_on, int cosine, int W, int T,
                                                  double lr_min, double eta, double wd, float* __restrict__ consts,
                                                  float* __restrict__ trust) {
    __shared__ double red[4];
    __shared__ float clip;
    double s = 0.0;
    if (clip_on)
        for (int i = threadIdx.x; i < np; i += 256) s += partial_g[i];
    s = wg256_sum_f64(s, red);
    if (threadIdx.x == 0) {
        const float t = step[0] + 1.f;
        step[0] = t;
        const double lr_t = scheduled_lr((double)lr[0], (double)t, cosine, W, T, lr_min);
        double norm = 0.0, c = 1.0;
        if (clip_on) {
            norm = sqrt(s);
            c = max_norm / (norm + 1e-6);
            if (c > 1.0) c = 1.0;
        }
        consts[0] = (float)lr_t;
        consts[1] = 0.f;
        consts[2] = (float)lr_t;
        consts[3] = (float)c;
        consts[4] = (float)norm;
        clip = (float)c;
    }
    if (px.nt == 0) return;                                   // uniform: plain SGD
    __syncthreads();
    const double c = (double)clip;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < px.nt; i += 4) {
        double sp = 0.0, sg = 0.0;
        for (int k = px.chunk0[i] + lane; k < px.chunk0[i + 1]; k += 64) {
            sp += partial_p[k];
            sg += partial_g[k];
        }
        sp = wave_sum_f64(sp);
        sg = wave_sum_f64(sg);
        if (lane == 0) {
            const double wn = sqrt(sp), gn = c * sqrt(sg);
            // a NaN norm fails the comparisons: ratio 1, and the NaN reaches the parameters through the gradient itself
            trust[i] = (px.mask[i] && wn > 0.0 && gn > 0.0) ? (float)(eta * wn / (gn + wd * wn)) : 1.f;
        }
    }
}

// d = c g (+ wd p on the flagged tensors), times the tensor's trust ratio; buf = mu buf + d; p -= lr_t (buf, or d + mu buf under
// Nesterov): torch.optim.SGD(momentum = mu, dampening = 0) in its operation order, one rounding per operation (the build has
// -ffp-contract=off).  c == 1.0f and q == 1.0f multiply exactly, so plain SGD pays nothing for the recipe's slots.
__global__ __launch_bounds__(256) void k_sgd_apply(SgdTable ts, const float* __restrict__ consts, const float* __restrict__ trust,
                                                   float mu, float wd, int nesterov) {
    const float lr_t = consts[2], c = consts[3];              // read while the search runs
    const Chunk ck = chunk_of(ts.t);
    const float q = trust ? trust[ck.t] : 1.f;
    const bool decay = ts.mask[ck.t];
    float* const col[3] = {ts.t.col[1][ck.t], ts.t.col[2][ck.t], ts.t.col[0][ck.t]};          // g, buf, p
    chunk_walk<0b110>(col, ck, [&](float (&x)[3][4], int E) {
        for (int e = 0; e < E; ++e) {
            const float gc = x[0][e] * c, p = x[2][e];
            float d = decay ? gc + wd * p : gc;
            d = d * q;
            const float buf = mu * x[1][e] + d;
            x[1][e] = buf;
            x[2][e] = p - lr_t * (nesterov ? d + mu * buf : buf);
        }
    });
}

}  // namespace

extern "C" int facl_adam_prep(const float* lr, float* step, float b1, float b2, float* consts, void* stream) {
    if (!lr || !step || !consts) return FACL_E_NULL;
    hipLaunchKernelGGL(k_adam_prep, dim3(1), dim3(64), 0, (hipStream_t)stream, lr, step, b1, b2, consts);
    return facl_launch_status();
}

// p / g / m / v: HOST arrays of nt device pointers; n: HOST array of element counts
extern "C" int facl_adam_apply(int nt, float* const* p, const float* const* g, float* const* m, float* const* v, const int* n,
                               const float* consts, float b1, float b2, float eps, void* stream) {
    if (!consts) return FACL_E_NULL;
    ChunkTable<4> tb;
    const int chunks = chunk_table(tb, nt, {p, g, m, v}, n);
    if (chunks < 0) return chunks;
    hipLaunchKernelGGL(k_adam_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, consts, b1, b2, eps);
    return facl_launch_status();
}

// pk / p: HOST arrays of nt device pointers (the averaged copy, the trained parameter); n: HOST array of element counts
extern "C" int facl_ema_apply(int nt, float* const* pk, const float* const* p, const int* n, float m, void* stream) {
    if (!(m >= 0.f && m <= 1.f)) return FACL_E_SHAPE;            // NaN included
    ChunkTable<2> tb;
    const int chunks = chunk_table(tb, nt, {pk, p}, n);
    if (chunks < 0) return chunks;
    hipLaunchKernelGGL(k_ema_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, m);
    return facl_launch_status();
}

// g: HOST array of nt device pointers; n: HOST array of element counts; partial: DEVICE array of one double per chunk
// (sum over i of ceil(n[i] / FACL_ADAM_CHUNK)), every entry written
extern "C" int facl_grad_sqnorm(int nt, const float* const* g, const int* n, double* partial, void* stream) {
    if (!partial) return FACL_E_NULL;
    ChunkTable<1> tb;
    const int chunks = chunk_table(tb, nt, {g}, n);
    if (chunks < 0) return chunks;
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, partial);
    return facl_launch_status();
}

extern "C" int facl_adam_prep_ex(const float* lr, float* step, float b1, float b2, const double* partial, int npartial,
                                 double max_norm, int schedule, int warmup_steps, int decay_steps, double lr_min, float* consts,
                                 void* stream) {
    if (!lr || !step || !consts || (npartial > 0 && !partial)) return FACL_E_NULL;
    if (npartial < 0 || (npartial > 0 && !(max_norm > 0.0))) return FACL_E_SHAPE;              // NaN included
    if (schedule != FACL_LR_STEP && schedule != FACL_LR_COSINE) return FACL_E_SHAPE;
    if (warmup_steps < 0 || !(lr_min >= 0.0)) return FACL_E_SHAPE;
    if (schedule == FACL_LR_COSINE && decay_steps <= warmup_steps) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_adam_prep_ex, dim3(1), dim3(256), 0, (hipStream_t)stream, lr, step, b1, b2, partial, npartial, max_norm,
                       schedule == FACL_LR_COSINE ? 1 : 0, warmup_steps, decay_steps, lr_min, consts);
    return facl_launch_status();
}

// p / g / m / v / n as in facl_adam_apply; decay: HOST array of nt flags (non-zero: the tensor is decayed)
extern "C" int facl_adamw_apply(int nt, float* const* p, const float* const* g, float* const* m, float* const* v, const int* n,
                                const int* decay, const float* consts, float b1, float b2, float eps, float wd, void* stream) {
    if (!decay || !consts) return FACL_E_NULL;
    if (!(wd >= 0.f)) return FACL_E_SHAPE;                       // NaN included
    AdamWTable tw;
    const int chunks = chunk_table(tw.t, nt, {p, g, m, v}, n);
    if (chunks < 0) return chunks;
    for (int i = 0; i < nt; ++i) tw.decay[i] = decay[i] ? 1 : 0;
    hipLaunchKernelGGL(k_adamw_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tw, consts, b1, b2, eps, wd);
    return facl_launch_status();
}

// p / g: HOST arrays of nt device pointers; n: HOST array of element counts; partial_p / partial_g: DEVICE arrays of one double
// per chunk, every entry written
extern "C" int facl_tensor_sqnorms(int nt, const float* const* p, const float* const* g, const int* n, double* partial_p,
                                   double* partial_g, void* stream) {
    if (!partial_p || !partial_g) return FACL_E_NULL;
    ChunkTable<2> tb;
    const int chunks = chunk_table(tb, nt, {p, g}, n);
    if (chunks < 0) return chunks;
    hipLaunchKernelGGL(k_tensor_sqnorms, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, partial_p, partial_g);
    return facl_launch_status();
}

// partial_p != NULL: LARS; then n (HOST, nt element counts) and mask (HOST, nt flags) describe the tensors whose partials the two
// arrays hold, npartial is their chunk count, and trust (DEVICE, nt floats) is written.  partial_p == NULL: nt, n, mask, eta, wd
// and trust are not read.
extern "C" int facl_sgd_prep(const float* lr, float* step, const double* partial_g, const double* partial_p, int npartial, int nt,
                             const int* n, const int* mask, double max_norm, int clip_on, int schedule, int warmup_steps,
                             int decay_steps, double lr_min, double eta, double wd, float* consts, float* trust, void* stream) {
    if (!lr || !step || !consts) return FACL_E_NULL;
    if (!partial_g && (clip_on || partial_p)) return FACL_E_NULL;
    if (partial_p && (!n || !mask || !trust)) return FACL_E_NULL;
    if (npartial < 0 || (clip_on && !(max_norm > 0.0))) return FACL_E_SHAPE;                   // NaN included
    if (schedule != FACL_LR_STEP && schedule != FACL_LR_COSINE) return FACL_E_SHAPE;
    if (warmup_steps < 0 || !(lr_min >= 0.0)) return FACL_E_SHAPE;
    if (schedule == FACL_LR_COSINE && decay_steps <= warmup_steps) return FACL_E_SHAPE;
    SgdPrefix px;
    px.nt = 0;
    if (partial_p) {
        if (!(eta >= 0.0) || !(wd >= 0.0)) return FACL_E_SHAPE;
        if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
        int chunks = 0;
        for (int i = 0; i < nt; ++i) {
            if (n[i] < 1) return FACL_E_SHAPE;
            px.chunk0[i] = chunks;
            px.mask[i] = mask[i] ? 1 : 0;
            chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
        }
        px.chunk0[nt] = chunks;
        if (chunks != npartial) return FACL_E_SHAPE;          // the partials are those of these tensors
        px.nt = nt;
    }
    hipLaunchKernelGGL(k_sgd_prep, dim3(1), dim3(256), 0, (hipStream_t)stream, lr, step, partial_g, partial_p, npartial, px,
                       max_norm, clip_on ? 1 : 0, schedule == FACL_LR_COSINE ? 1 : 0, warmup_steps, decay_steps, lr_min, eta, wd,
                       consts, trust);
    return facl_launch_status();
}

// p / g / buf: HOST arrays of nt device pointers (parameter, gradient, momentum buffer); n, mask: HOST arrays of element counts
// and flags; consts: facl_sgd_prep's; trust: its ratios, or NULL = 1 for every tensor
extern "C" int facl_sgd_apply(int nt, float* const* p, const float* const* g, float* const* buf, const int* n, const int* mask,
                              const float* consts, const float* trust, float mu, float wd, int nesterov, void* stream) {
    if (!mask || !consts) return FACL_E_NULL;
    if (!(mu >= 0.f && mu < 1.f) || !(wd >= 0.f)) return FACL_E_SHAPE;                         // NaN included
    SgdTable ts;
    const int chunks = chunk_table(ts.t, nt, {p, g, buf}, n);
    if (chunks < 0) return chunks;
    for (int i = 0; i < nt; ++i) ts.mask[i] = mask[i] ? 1 : 0;
    hipLaunchKernelGGL(k_sgd_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, ts, consts, trust, mu, wd, nesterov ? 1 : 0);
    return facl_launch_status();
}
