// Adam step of the training loop (cn3d_train_motion_GL.py:180,:332: torch.optim.Adam(lr 3e-4, betas (0.5, 0.999), eps 1e-6),
// no weight decay, no amsgrad) for ALL parameters in one launch.  torch's fused multi-tensor kernel walks 64 K-element
// chunks: 2.36 M parameters are 36 workgroups (47 us on 256 CUs); here a workgroup takes 2048 elements (~1150 workgroups,
// HBM-bound: 7 x 9.4 MB per step).  Tensor pointers travel BY VALUE in the kernel arguments (no device-side table to keep
// coherent; a HIP graph bakes them at capture time, when the gradient buffers of the captured step are fixed).
//   facl_adam_prep: step += 1; consts = (lr / (1 - b1^t), 1 / sqrt(1 - b2^t))      -- one thread, device-resident lr / step
//   facl_adam_apply: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
// and the momentum average of the key encoder that follows it in the step (facl_amd/key_encoder.py; MoCo's
// _momentum_update_key_encoder: param_k = param_k * m + param_q * (1 - m), parameters only), same table, same chunks:
//   facl_ema_apply: pk = m pk + (1-m) p
// and the optimizer recipe of the contrastive modes (facl_amd/optim.py: weight_decay, max_grad_norm, schedule), off by
// default -- the three entries above are then the whole step, unchanged:
//   facl_grad_sqnorm: partial[chunk] = sum of g^2 over the chunk in fp64, fixed order, no atomics  -- only when clipping
//   facl_adam_prep_ex: step += 1; norm = sqrt(sum of the partials), c = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_);
//                      lr_t = warm-up x (host lr | cosine) from the step counter; consts = (lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t),
//                      lr_t, c, norm)
//   facl_adamw_apply: g' = c g; p *= 1 - lr_t wd on flagged tensors (torch.optim.AdamW's order); then facl_adam_apply's update on g'
#include "common.h"
#include <math.h>
#include <stdint.h>

#define FACL_ADAM_MAX_TENSORS 64
#define FACL_ADAM_CHUNK 2048

struct FaclAdamTable {
    float* p[FACL_ADAM_MAX_TENSORS];
    const float* g[FACL_ADAM_MAX_TENSORS];
    float* m[FACL_ADAM_MAX_TENSORS];
    float* v[FACL_ADAM_MAX_TENSORS];
    int n[FACL_ADAM_MAX_TENSORS];
    int chunk0[FACL_ADAM_MAX_TENSORS + 1];        // first chunk of tensor i (prefix sums of ceil(n / CHUNK))
    int nt;
};

struct FaclAdamWTable {
    FaclAdamTable t;
    unsigned char decay[FACL_ADAM_MAX_TENSORS];   // 1: the tensor is weight-decayed
};

struct FaclGradTable {
    const float* g[FACL_ADAM_MAX_TENSORS];
    int n[FACL_ADAM_MAX_TENSORS];
    int chunk0[FACL_ADAM_MAX_TENSORS + 1];
    int nt;
};

struct FaclEmaTable {
    float* pk[FACL_ADAM_MAX_TENSORS];
    const float* p[FACL_ADAM_MAX_TENSORS];
    int n[FACL_ADAM_MAX_TENSORS];
    int chunk0[FACL_ADAM_MAX_TENSORS + 1];
    int nt;
};

namespace {

__global__ void k_adam_prep(const float* __restrict__ lr, float* __restrict__ step, float b1, float b2,
                            float* __restrict__ consts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float t = step[0] + 1.f;
    step[0] = t;
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    consts[0] = (float)((double)lr[0] / bc1);
    consts[1] = (float)(1.0 / sqrt(bc2));
}

__global__ __launch_bounds__(256) void k_adam_apply(FaclAdamTable tb, const float* __restrict__ consts, float b1, float b2,
                                                    float eps) {
    // tensor of this chunk: binary search in the prefix table (wave-uniform)
    int lo = 0, hi = tb.nt;
    const int c = blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int t = lo, base = (c - tb.chunk0[t]) * FACL_ADAM_CHUNK;
    const int n = tb.n[t];
    float* __restrict__ p = tb.p[t];
    const float* __restrict__ g = tb.g[t];
    float* __restrict__ m = tb.m[t];
    float* __restrict__ v = tb.v[t];
    const float step_size = consts[0], isb2 = consts[1];
    // 16 bytes per lane where the tensor allows it (every tensor of the model does): a quarter of the memory instructions of the
    // scalar walk below, all of a thread's loads in flight before its first store
    if (!(n & 3) && !((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15)) {
        float4 g4[2], m4[2], v4[2], p4[2];
        int i4[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            i4[k] = (base >> 2) + k * 256 + threadIdx.x;
            if (4 * i4[k] < n) {
                g4[k] = reinterpret_cast<const float4*>(g)[i4[k]]; m4[k] = reinterpret_cast<const float4*>(m)[i4[k]];
                v4[k] = reinterpret_cast<const float4*>(v)[i4[k]]; p4[k] = reinterpret_cast<const float4*>(p)[i4[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (4 * i4[k] >= n) continue;
            float gg[4] = {g4[k].x, g4[k].y, g4[k].z, g4[k].w}, mm[4] = {m4[k].x, m4[k].y, m4[k].z, m4[k].w};
            float vv[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w}, pp[4] = {p4[k].x, p4[k].y, p4[k].z, p4[k].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float mi = b1 * mm[e] + (1.f - b1) * gg[e];
                const float vi = b2 * vv[e] + (1.f - b2) * gg[e] * gg[e];
                mm[e] = mi; vv[e] = vi;
                pp[e] -= step_size * (mi / (sqrtf(vi) * isb2 + eps));
            }
            reinterpret_cast<float4*>(m)[i4[k]] = make_float4(mm[0], mm[1], mm[2], mm[3]);
            reinterpret_cast<float4*>(v)[i4[k]] = make_float4(vv[0], vv[1], vv[2], vv[3]);
            reinterpret_cast<float4*>(p)[i4[k]] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < FACL_ADAM_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const float gi = g[i];
            const float mi = b1 * m[i] + (1.f - b1) * gi;
            const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            p[i] -= step_size * (mi / (sqrtf(vi) * isb2 + eps));
        }
    }
}

// pk = m pk + (1-m) p.  Three roundings and the one of 1 - m (the build has -ffp-contract=off); m = 0 copies p and m = 1 leaves pk
// as it is through the formula itself: 0 * finite = 0, x + 0 = x.
__global__ __launch_bounds__(256) void k_ema_apply(FaclEmaTable tb, float m) {
    int lo = 0, hi = tb.nt;
    const int c = blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int t = lo, base = (c - tb.chunk0[t]) * FACL_ADAM_CHUNK;
    const int n = tb.n[t];
    float* __restrict__ pk = tb.pk[t];
    const float* __restrict__ p = tb.p[t];
    const float om = 1.f - m;
    if (!(n & 3) && !((((uintptr_t)pk) | ((uintptr_t)p)) & 15)) {
        float4 k4[2], p4[2];
        int i4[2];
        const int n4 = n >> 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            i4[k] = (base >> 2) + k * 256 + threadIdx.x;
            if (i4[k] < n4) {
                k4[k] = reinterpret_cast<const float4*>(pk)[i4[k]]; p4[k] = reinterpret_cast<const float4*>(p)[i4[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (i4[k] >= n4) continue;
            reinterpret_cast<float4*>(pk)[i4[k]] = make_float4(m * k4[k].x + om * p4[k].x, m * k4[k].y + om * p4[k].y,
                                                               m * k4[k].z + om * p4[k].z, m * k4[k].w + om * p4[k].w);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < FACL_ADAM_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) pk[i] = m * pk[i] + om * p[i];
    }
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
// significant bits and is exact in fp64, so the only roundings are those of the additions, whose order is fixed by (chunk, thread).
__global__ __launch_bounds__(256) void k_grad_sqnorm(FaclGradTable tb, double* __restrict__ partial) {
    __shared__ double red[4];
    int lo = 0, hi = tb.nt;
    const int c = blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int t = lo, base = (c - tb.chunk0[t]) * FACL_ADAM_CHUNK;
    const int n = tb.n[t];
    const float* __restrict__ g = tb.g[t];
    double s = 0.0;
    if (!(n & 3) && !(((uintptr_t)g) & 15)) {
        float4 g4[2];
        int i4[2];
        const int n4 = n >> 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            i4[k] = (base >> 2) + k * 256 + threadIdx.x;
            if (i4[k] < n4) g4[k] = reinterpret_cast<const float4*>(g)[i4[k]];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (i4[k] >= n4) continue;
            const double x = g4[k].x, y = g4[k].y, z = g4[k].z, w = g4[k].w;
            s += ((x * x + y * y) + z * z) + w * w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < FACL_ADAM_CHUNK / 256; ++k) {
            const int i = base + k * 256 + threadIdx.x;
            if (i < n) { const double x = g[i]; s += x * x; }
        }
    }
    s = wg256_sum_f64(s, red);
    if (threadIdx.x == 0) partial[c] = s;
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
    const float t = step[0] + 1.f;
    step[0] = t;
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    const double tt = (double)t, lr0 = (double)lr[0];
    const double warm = W > 0 ? fmin(1.0, tt / (double)W) : 1.0;
    double lr_s = lr0;
    if (cosine) {
        const double tp = fmax(tt - (double)W, 0.0), Tp = (double)(T - W);
        lr_s = lr_min + (lr0 - lr_min) * 0.5 * (1.0 + cos(M_PI * fmin(tp, Tp) / Tp));
    }
    const double lr_t = warm * lr_s;
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

// k_adam_apply with the clip coefficient on the gradient VALUE (p.grad is only read) and the decoupled decay in front of the
// update.  With c == 1.0f and wd == 0 every product added here is x * 1.0f, which is exact: the outputs are k_adam_apply's bits
// (the remaining expressions are its own, in its order; the build has -ffp-contract=off).
__global__ __launch_bounds__(256) void k_adamw_apply(FaclAdamWTable tw, const float* __restrict__ consts, float b1, float b2,
                                                     float eps, float wd) {
    const FaclAdamTable& tb = tw.t;
    int lo = 0, hi = tb.nt;
    const int c = blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int t = lo, base = (c - tb.chunk0[t]) * FACL_ADAM_CHUNK;
    const int n = tb.n[t];
    float* __restrict__ p = tb.p[t];
    const float* __restrict__ g = tb.g[t];
    float* __restrict__ m = tb.m[t];
    float* __restrict__ v = tb.v[t];
    const float step_size = consts[0], isb2 = consts[1], clip = consts[3];
    const float keep = tw.decay[t] ? 1.f - consts[2] * wd : 1.f;           // torch.optim.AdamW: param.mul_(1 - lr * weight_decay)
    if (!(n & 3) && !((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15)) {
        float4 g4[2], m4[2], v4[2], p4[2];
        int i4[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            i4[k] = (base >> 2) + k * 256 + threadIdx.x;
            if (4 * i4[k] < n) {
                g4[k] = reinterpret_cast<const float4*>(g)[i4[k]]; m4[k] = reinterpret_cast<const float4*>(m)[i4[k]];
                v4[k] = reinterpret_cast<const float4*>(v)[i4[k]]; p4[k] = reinterpret_cast<const float4*>(p)[i4[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (4 * i4[k] >= n) continue;
            float gg[4] = {g4[k].x, g4[k].y, g4[k].z, g4[k].w}, mm[4] = {m4[k].x, m4[k].y, m4[k].z, m4[k].w};
            float vv[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w}, pp[4] = {p4[k].x, p4[k].y, p4[k].z, p4[k].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gi = gg[e] * clip;
                const float mi = b1 * mm[e] + (1.f - b1) * gi;
                const float vi = b2 * vv[e] + (1.f - b2) * gi * gi;
                mm[e] = mi; vv[e] = vi;
                pp[e] = pp[e] * keep;
                pp[e] -= step_size * (mi / (sqrtf(vi) * isb2 + eps));
            }
            reinterpret_cast<float4*>(m)[i4[k]] = make_float4(mm[0], mm[1], mm[2], mm[3]);
            reinterpret_cast<float4*>(v)[i4[k]] = make_float4(vv[0], vv[1], vv[2], vv[3]);
            reinterpret_cast<float4*>(p)[i4[k]] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < FACL_ADAM_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const float gi = g[i] * clip;
            const float mi = b1 * m[i] + (1.f - b1) * gi;
            const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            const float pi = p[i] * keep;
            p[i] = pi - step_size * (mi / (sqrtf(vi) * isb2 + eps));
        }
    }
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
    if (!p || !g || !m || !v || !n || !consts) return FACL_E_NULL;
    if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
    FaclAdamTable tb;
    int chunks = 0;
    for (int i = 0; i < nt; ++i) {
        if (!p[i] || !g[i] || !m[i] || !v[i]) return FACL_E_NULL;
        if (n[i] < 1) return FACL_E_SHAPE;
        tb.p[i] = p[i]; tb.g[i] = g[i]; tb.m[i] = m[i]; tb.v[i] = v[i]; tb.n[i] = n[i];
        tb.chunk0[i] = chunks;
        chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
    }
    tb.chunk0[nt] = chunks;
    tb.nt = nt;
    hipLaunchKernelGGL(k_adam_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, consts, b1, b2, eps);
    return facl_launch_status();
}

// pk / p: HOST arrays of nt device pointers (the averaged copy, the trained parameter); n: HOST array of element counts
extern "C" int facl_ema_apply(int nt, float* const* pk, const float* const* p, const int* n, float m, void* stream) {
    if (!pk || !p || !n) return FACL_E_NULL;
    if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
    if (!(m >= 0.f && m <= 1.f)) return FACL_E_SHAPE;            // NaN included
    FaclEmaTable tb;
    int chunks = 0;
    for (int i = 0; i < nt; ++i) {
        if (!pk[i] || !p[i]) return FACL_E_NULL;
        if (n[i] < 1) return FACL_E_SHAPE;
        tb.pk[i] = pk[i]; tb.p[i] = p[i]; tb.n[i] = n[i];
        tb.chunk0[i] = chunks;
        chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
    }
    tb.chunk0[nt] = chunks;
    tb.nt = nt;
    hipLaunchKernelGGL(k_ema_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tb, m);
    return facl_launch_status();
}

// g: HOST array of nt device pointers; n: HOST array of element counts; partial: DEVICE array of one double per 2048-element chunk
// (sum over i of ceil(n[i] / 2048)), every entry written
extern "C" int facl_grad_sqnorm(int nt, const float* const* g, const int* n, double* partial, void* stream) {
    if (!g || !n || !partial) return FACL_E_NULL;
    if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
    FaclGradTable tb;
    int chunks = 0;
    for (int i = 0; i < nt; ++i) {
        if (!g[i]) return FACL_E_NULL;
        if (n[i] < 1) return FACL_E_SHAPE;
        tb.g[i] = g[i]; tb.n[i] = n[i];
        tb.chunk0[i] = chunks;
        chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
    }
    tb.chunk0[nt] = chunks;
    tb.nt = nt;
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
    if (!p || !g || !m || !v || !n || !decay || !consts) return FACL_E_NULL;
    if (nt < 1 || nt > FACL_ADAM_MAX_TENSORS) return FACL_E_SHAPE;
    if (!(wd >= 0.f)) return FACL_E_SHAPE;                       // NaN included
    FaclAdamWTable tw;
    FaclAdamTable& tb = tw.t;
    int chunks = 0;
    for (int i = 0; i < nt; ++i) {
        if (!p[i] || !g[i] || !m[i] || !v[i]) return FACL_E_NULL;
        if (n[i] < 1) return FACL_E_SHAPE;
        tb.p[i] = p[i]; tb.g[i] = g[i]; tb.m[i] = m[i]; tb.v[i] = v[i]; tb.n[i] = n[i];
        tw.decay[i] = decay[i] ? 1 : 0;
        tb.chunk0[i] = chunks;
        chunks += (n[i] + FACL_ADAM_CHUNK - 1) / FACL_ADAM_CHUNK;
    }
    tb.chunk0[nt] = chunks;
    tb.nt = nt;
    hipLaunchKernelGGL(k_adamw_apply, dim3(chunks), dim3(256), 0, (hipStream_t)stream, tw, consts, b1, b2, eps, wd);
    return facl_launch_status();
}
