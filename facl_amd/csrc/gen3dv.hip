// Depth frames -> 3DV point clouds (the reference's generate_data/generate_NTU.py) for a batch of clips.
//
// Stages, one entry point each (include/facl_hip.h, "3DV generation"; facl_amd/gen3dv.py drives them):
//   frames    per frame: the crop box of load_depth_from_img (:339-351) as a predicate, the number of pixels it keeps, and
//             the float64 extents of their back-projection (:321-335)
//   voxelise  per chosen frame: bit i of a 64-bit word per voxel for "frame i has a point here" (full image and motion
//             image, :355-366, :393-407), and the row-major list of the kept pixels (the appearance clouds draw ranks)
//   volumes   per voxel: the five rank-pooling channels and the key value from the set bits and a weight table (:409-438)
//   filter    per voxel: disca_voxel (:277-296) on channel 0 (threshold 5) and on the key volume (threshold 6)
//   compact   per clip: the (m,x,y,z)-ordered hits and the (x,y,z)-ordered unique voxels of the 5-channel volume and of the
//             key-masked volume (:196-201, :212-219), and their four counts
//   sample    per clip: 2048 rows of each cloud by drawn index, extents, normalisation (:203-247)
//   app       per appearance frame: 2048 drawn points, their unrounded voxel coordinates and channel 0 (:49-74, :249-260)
//
// Arithmetic that decides a voxel or an output value is float64 in the reference's operation order; the library is built
// with -ffp-contract=off (facl_amd/build.py), so a multiply and a divide stay two roundings.  Volumes are int32: every
// value is a sum of at most 64 weights below 64 in magnitude.
//
// Layouts (all int32 unless said otherwise):
//   frames  uint16 (NF, H, W): per clip its folder's first file, then its chosen frames
//   fmeta   (NF, 4): clip, bit (index among the clip's chosen frames, -1 for the first file), frame that precedes it in
//           the motion chain, offset of its pixel list in pix
//   fbox    (NF, 4): kept rows are [60, rhi), kept columns [clo, chi); fbox[3] = 1 if the frame has a non-zero pixel
//   cgrid   (B, 4): nx, ny, nz, offset of the clip's voxels; voxel (x, y, z) is (x * ny + y) * nz + z
//   cmin    float64 (B, 3): the bounding box's minimum
//   vol     (5, NV): channel planes over all voxels of the batch; vol0f (NV) the filtered channel 0; keyf (NV)
//   lists   (12 * NV): per clip at 12 * offset: hits (5 V), unique (V), key hits (5 V), key unique (V), local voxel numbers
//   counts  (B, 4) in that order
#include "common.h"

namespace {

constexpr double FX = 365.481, FY = 365.481, CX = 257.346, CY = 210.347;      // generate_NTU.py:14-17
constexpr int TOP = 60, BOTTOM = 29, SIDE = 10, LOW = 50, UP = 300;         // :31, :356-357
constexpr int NS = 2048;                                                      // SAMPLE_NUM
constexpr int TH = 1024, NW = TH / FACL_WAVE;                                 // threads / waves of the per-frame and per-clip kernels

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// Python's a[s:] for a start that may be negative
__device__ __forceinline__ int slice_start(int s, int n) {
    if (s < 0) s += n;
    return s < 0 ? 0 : (s > n ? n : s);
}

__device__ __forceinline__ bool in_box(const int* box, int r, int c) {
    return r >= TOP && r < box[0] && c >= box[1] && c < box[2];
}

__device__ __forceinline__ void backproject(int r, int c, int d, double& X, double& Y, double& Z) {
    X = ((double)c - CX) * (double)d / FX;
    Y = ((double)r - CY) * (double)d / FY;
    Z = (double)d;
}

// ---- frames ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_frames(const uint16_t* __restrict__ frames, int H, int W, int* __restrict__ fbox,
                                               int* __restrict__ fcount, double* __restrict__ fext) {
    __shared__ int s_i[3];
    __shared__ int s_box[4];
    __shared__ int s_cnt[NW];
    __shared__ double s_ext[6][NW];
    const int g = blockIdx.x, t = threadIdx.x, w = t / FACL_WAVE, P = H * W;
    const uint16_t* im = frames + (size_t)g * P;
    if (t == 0) { s_i[0] = -1; s_i[1] = W; s_i[2] = -1; }
    __syncthreads();
    int rl = -1, cl = W, ch = -1;                        // last row, first / last column of the non-zero pixels off the border
    for (int p = t; p < P; p += TH) {
        const int r = p / W, c = p - r * W;
        if (r >= 2 && c >= 2 && im[p] != 0) { rl = max(rl, r); cl = min(cl, c); ch = max(ch, c); }
    }
    rl = wave_max_i32(rl); cl = wave_min_i32(cl); ch = wave_max_i32(ch);
    if (lane_id() == 0) { atomicMax(&s_i[0], rl); atomicMin(&s_i[1], cl); atomicMax(&s_i[2], ch); }
    __syncthreads();
    if (t == 0) {
        const bool any = s_i[0] >= 0;
        s_box[0] = any ? slice_start(s_i[0] - BOTTOM, H) : 0;
        s_box[1] = any ? s_i[1] + SIDE : 0;
        s_box[2] = any ? slice_start(s_i[2] - SIDE, W) : 0;
        s_box[3] = any ? 1 : 0;
        for (int k = 0; k < 4; ++k) fbox[g * 4 + k] = s_box[k];
    }
    __syncthreads();
    int cnt = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int p1 = min(s_box[0], H) * W;
    for (int p = TOP * W + t; p < p1; p += TH) {
        const int r = p / W, c = p - r * W, d = im[p];
        if (d != 0 && c >= s_box[1] && c < s_box[2]) {
            double v[3];
            backproject(r, c, d, v[0], v[1], v[2]);
            ++cnt;
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], v[k]); hi[k] = fmax(hi[k], v[k]); }
        }
    }
    cnt = wave_sum_i32(cnt);
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = wave_min_f64(lo[k]); hi[k] = wave_max_f64(hi[k]); }
    if (lane_id() == 0) {
        s_cnt[w] = cnt;
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_ext[k][w] = lo[k]; s_ext[3 + k][w] = hi[k]; }
    }
    __syncthreads();
    if (t == 0) {
        int c = 0;
        for (int k = 0; k < NW; ++k) c += s_cnt[k];
        fcount[g] = c;
    }
    if (t < 6) {
        double v = s_ext[t][0];
        for (int k = 1; k < NW; ++k) v = t < 3 ? fmin(v, s_ext[t][k]) : fmax(v, s_ext[t][k]);
        fext[g * 6 + t] = v;
    }
}

// ---- voxelise --------------------------------------------------------------------------------------------------------------
constexpr int E_VOXEL = 1, E_PIXEL = 2, E_BIT = 4, E_EMPTY = 8, E_INDEX = 16;      // bits of *err

__global__ __launch_bounds__(TH) void k_voxelise(const uint16_t* __restrict__ frames, int NF, int H, int W,
                                                 const int* __restrict__ fbox, const int* __restrict__ fmeta,
                                                 const double* __restrict__ cmin, const int* __restrict__ cgrid, int B,
                                                 int maxF, long long NV, long long NP, double voxel,
                                                 unsigned long long* __restrict__ occ,
                                                 unsigned long long* __restrict__ mocc, int* __restrict__ pix,
                                                 int* __restrict__ err) {
    __shared__ int wtot[NW];
    const int g = blockIdx.x, t = threadIdx.x, w = t / FACL_WAVE, P = H * W;
    const int b = fmeta[g * 4], bit = fmeta[g * 4 + 1], gp = fmeta[g * 4 + 2], poff = fmeta[g * 4 + 3];
    if (bit < 0) return;                                            // a folder's first file: only ever a `prev`
    if (bit >= maxF || bit >= 64 || b < 0 || b >= B || gp < 0 || gp >= NF || poff < 0) {
        if (t == 0) atomicOr(err, E_BIT);
        return;
    }
    const uint16_t* im = frames + (size_t)g * P;
    const uint16_t* pim = frames + (size_t)gp * P;
    int box[3] = {fbox[g * 4], fbox[g * 4 + 1], fbox[g * 4 + 2]};
    int pbox[3] = {fbox[gp * 4], fbox[gp * 4 + 1], fbox[gp * 4 + 2]};
    const double m0 = cmin[b * 3], m1 = cmin[b * 3 + 1], m2 = cmin[b * 3 + 2];
    const int nx = cgrid[b * 4], ny = cgrid[b * 4 + 1], nz = cgrid[b * 4 + 2];
    const long long voff = cgrid[b * 4 + 3];
    const unsigned long long below = lanemask_lt(), mybit = 1ull << bit;
    int run = 0;                                                    // pixels kept so far (uniform across the block)
    const int p1 = min(box[0], H) * W;
    for (int p0 = TOP * W; p0 < p1; p0 += TH) {
        const int p = p0 + t;
        bool keep = false;
        int r = 0, c = 0, d = 0;
        if (p < p1) {
            r = p / W; c = p - r * W; d = im[p];
            keep = d != 0 && c >= box[1] && c < box[2];
        }
        const unsigned long long m = __ballot(keep);
        if (lane_id() == 0) wtot[w] = __popcll(m);
        __syncthreads();
        int off = run, tot = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { if (k < w) off += wtot[k]; tot += wtot[k]; }
        if (keep) {
            const long long slot = (long long)poff + off + __popcll(m & below);
            if (slot < NP) pix[slot] = p; else atomicOr(err, E_PIXEL);
            double X, Y, Z;
            backproject(r, c, d, X, Y, Z);
            const int ix = (int)((X - m0) / voxel), iy = (int)((Y - m1) / voxel), iz = (int)((Z - m2) / voxel);
            const long long v = voff + ((long long)ix * ny + iy) * nz + iz;
            if (ix < 0 || ix >= nx || iy < 0 || iy >= ny || iz < 0 || iz >= nz || v >= NV) {
                atomicOr(err, E_VOXEL);
            } else {
                atomicOr(&occ[v], mybit);
                const int pd = in_box(pbox, r, c) ? (int)pim[p] : 0;
                const int diff = abs(d - pd);
                if (diff > LOW && diff < UP) atomicOr(&mocc[v], mybit);
            }
        }
        run += tot;
        __syncthreads();                                            // wtot is rewritten by the next pass
    }
}

// ---- volumes ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_volumes(const unsigned long long* __restrict__ occ,
                                                 const unsigned long long* __restrict__ mocc,
                                                 const int* __restrict__ wtab, const int* __restrict__ cgrid, long long NV,
                                                 int* __restrict__ vol, int* __restrict__ key) {
    __shared__ int s_w[5 * 64];
    const int b = blockIdx.y, t = threadIdx.x;
    for (int k = t; k < 5 * 64; k += 256) s_w[k] = wtab[b * 5 * 64 + k];
    __syncthreads();
    const int V = cgrid[b * 4] * cgrid[b * 4 + 1] * cgrid[b * 4 + 2];
    const int v = blockIdx.x * 256 + t;
    if (v >= V) return;
    const long long a = (long long)cgrid[b * 4 + 3] + v;
    if (a >= NV) return;
    int ch[5] = {0, 0, 0, 0, 0}, kv = 0;
    for (unsigned long long m = occ[a]; m; m &= m - 1) {
        const int i = __ffsll((long long)m) - 1;
#pragma unroll
        for (int c = 0; c < 5; ++c) ch[c] += s_w[c * 64 + i];
    }
    for (unsigned long long m = mocc[a]; m; m &= m - 1) kv += s_w[__ffsll((long long)m) - 1];
#pragma unroll
    for (int c = 0; c < 5; ++c) vol[c * NV + a] = ch[c];
    key[a] = kv;
}

// ---- filter ----------------------------------------------------------------------------------------------------------------
// Neighbour reads go through the cache: a clip's plane is a few hundred KB, every voxel of it is read 27 times by
// adjacent threads.
__global__ __launch_bounds__(256) void k_filter(const int* __restrict__ vol0, const int* __restrict__ key,
                                                const int* __restrict__ cgrid, long long NV, int th0, int thk,
                                                int* __restrict__ vol0f, int* __restrict__ keyf) {
    const int b = blockIdx.y;
    const int nx = cgrid[b * 4], ny = cgrid[b * 4 + 1], nz = cgrid[b * 4 + 2];
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nx * ny * nz) return;
    const long long base = cgrid[b * 4 + 3], a = base + v;
    if (a >= NV) return;
    const int z = v % nz, y = (v / nz) % ny, x = v / (nz * ny);
    int o0 = 0, ok = 0;
    if (x > 0 && x < nx - 1 && y > 0 && y < ny - 1 && z > 0 && z < nz - 1) {
        int n0 = 0, nk = 0;
        for (int i = -1; i <= 1; ++i)
            for (int j = -1; j <= 1; ++j)
                for (int k = -1; k <= 1; ++k) {
                    const long long q = base + ((long long)(x + i) * ny + (y + j)) * nz + (z + k);
                    n0 += vol0[q] != 0;
                    nk += key[q] != 0;
                }
        if (n0 >= th0) o0 = vol0[a];
        if (nk >= thk) ok = key[a];
    }
    vol0f[a] = o0;
    keyf[a] = ok;
}

// ---- compact ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int chan(const int* vol, const int* vol0f, long long NV, long long a, int m) {
    return m == 0 ? vol0f[a] : vol[m * NV + a];
}

// block (which, clip): which = 0 hits, 1 unique, 2 key hits, 3 key unique.  One workgroup walks its index space in order,
// 1024 entries per pass, and appends the flagged ones: the order of np.where / np.unique falls out of the walk.
__global__ __launch_bounds__(TH) void k_compact(const int* __restrict__ vol, const int* __restrict__ vol0f,
                                                const int* __restrict__ keyf, const int* __restrict__ cgrid, long long NV,
                                                int* __restrict__ lists, int* __restrict__ counts) {
    __shared__ int wtot[NW];
    const int which = blockIdx.x, b = blockIdx.y, t = threadIdx.x, w = t / FACL_WAVE;
    const int V = cgrid[b * 4] * cgrid[b * 4 + 1] * cgrid[b * 4 + 2];
    const long long base = cgrid[b * 4 + 3];
    const bool masked = which >= 2, uniq = which & 1;
    int* out = lists + 12 * base + (long long)V * (which == 0 ? 0 : which == 1 ? 5 : which == 2 ? 6 : 11);
    const long long n = uniq ? V : 5ll * V;
    const unsigned long long below = lanemask_lt();
    int run = 0;
    if (base + V > NV) { if (t == 0) counts[b * 4 + which] = 0; return; }
    for (long long e0 = 0; e0 < n; e0 += TH) {
        const long long e = e0 + t;
        bool flag = false;
        int v = 0;
        if (e < n) {
            v = (int)(e % V);
            const long long a = base + v;
            if (!masked || keyf[a] != 0) {
                if (uniq) {
                    for (int m = 0; m < 5; ++m) flag |= chan(vol, vol0f, NV, a, m) != 0;
                } else {
                    flag = chan(vol, vol0f, NV, a, (int)(e / V)) != 0;
                }
            }
        }
        const unsigned long long m = __ballot(flag);
        if (lane_id() == 0) wtot[w] = __popcll(m);
        __syncthreads();
        int off = run, tot = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { if (k < w) off += wtot[k]; tot += wtot[k]; }
        if (flag) out[off + __popcll(m & below)] = v;
        run += tot;
        __syncthreads();
    }
    if (t == 0) counts[b * 4 + which] = run;
}

// ---- draws -----------------------------------------------------------------------------------------------------------------
// Philox4x32-10 as in csrc/views_philox.hip; facl_amd/gen3dv.py restates the recipe:
//   key = (seed & 0xffffffff, seed >> 32), counter = (row n in 0..2047, slot, crc32 of the clip's name, resolution)
//   slot 0: word 0 -> motion cloud, word 1 -> key cloud; slot 2 + j: word 0 -> appearance frame j
//   row = (uint64(word) * count) >> 32; where the reference keeps the list and appends (fewer than 2048), row n < count is n
struct u32x4 { uint32_t w[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ int draw_row(uint32_t w, int count) {
    return (int)(((unsigned long long)w * (unsigned long long)(uint32_t)count) >> 32);
}

// ---- sample ----------------------------------------------------------------------------------------------------------------
constexpr int NORM = 14;        // per clip: centre xyz, y_len, c_min[5], c_len[5]

__global__ __launch_bounds__(TH) void k_sample(const int* __restrict__ vol, const int* __restrict__ vol0f,
                                               const int* __restrict__ lists, const int* __restrict__ counts,
                                               const int* __restrict__ cgrid, long long NV, const int* __restrict__ idx,
                                               uint32_t k0, uint32_t k1, uint32_t res, const uint32_t* __restrict__ crc,
                                               double* __restrict__ out_raw, double* __restrict__ out_key,
                                               double* __restrict__ norm, int* __restrict__ err) {
    __shared__ int s_lo[8][NW], s_hi[8][NW];
    __shared__ double s_n[NORM];
    const int b = blockIdx.x, t = threadIdx.x, w = t / FACL_WAVE;
    const int ny = cgrid[b * 4 + 1], nz = cgrid[b * 4 + 2];
    const int V = cgrid[b * 4] * ny * nz;
    const long long base = cgrid[b * 4 + 3];
    if (base + V > NV) { if (t == 0) atomicOr(err, E_VOXEL); return; }
    for (int cloud = 0; cloud < 2; ++cloud) {
        const int hits = counts[b * 4 + 2 * cloud], nu = counts[b * 4 + 2 * cloud + 1];
        const bool useu = hits > NS;
        const int R = useu ? nu : hits;
        if (R <= 0) { if (t == 0) atomicOr(err, E_EMPTY); return; }          // uniform: counts are per clip
        const int* list = lists + 12 * base + (long long)V * (cloud * 6 + (useu ? 5 : 0));
        int row[2][8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = t + h * TH;
            int i;
            if (idx) {
                i = idx[((size_t)b * 2 + cloud) * NS + n];
            } else if (hits < NS && n < hits) {
                i = n;
            } else {
                i = draw_row(philox4x32_10((uint32_t)n, 0u, crc[b], res, k0, k1).w[cloud], R);
            }
            if (i < 0 || i >= R) { atomicOr(err, E_INDEX); i = 0; }
            const int v = list[i];
            row[h][0] = v / (ny * nz); row[h][1] = (v / nz) % ny; row[h][2] = v % nz;
#pragma unroll
            for (int m = 0; m < 5; ++m) row[h][3 + m] = chan(vol, vol0f, NV, base + v, m);
        }
        if (cloud == 0) {                                            // the constants come from the sampled motion cloud
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int lo = wave_min_i32(min(row[0][c], row[1][c])), hi = wave_max_i32(max(row[0][c], row[1][c]));
                if (lane_id() == 0) { s_lo[c][w] = lo; s_hi[c][w] = hi; }
            }
            __syncthreads();
            if (t < 8) {
                int lo = s_lo[t][0], hi = s_hi[t][0];
                for (int k = 1; k < NW; ++k) { lo = min(lo, s_lo[t][k]); hi = max(hi, s_hi[t][k]); }
                const double dlo = (double)lo, dhi = (double)hi;
                if (t < 3) s_n[t] = (dhi + dlo) / 2.0;
                if (t == 1) s_n[3] = dhi - dlo;
                if (t >= 3) { s_n[4 + (t - 3)] = dlo; s_n[9 + (t - 3)] = dhi - dlo; }
            }
            __syncthreads();
            if (t < NORM) norm[b * NORM + t] = s_n[t];
        }
        double* out = (cloud == 0 ? out_raw : out_key) + (size_t)b * NS * 8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double* o = out + (size_t)(t + h * TH) * 8;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = ((double)row[h][c] - s_n[c]) / s_n[3];
#pragma unroll
            for (int c = 0; c < 5; ++c) o[3 + c] = ((double)row[h][3 + c] - s_n[4 + c]) / s_n[9 + c] - 0.5;
        }
    }
}

// ---- app -------------------------------------------------------------------------------------------------------------------
// ameta (NA, 3): frame, clip, slot of the appearance frame within its clip
__global__ __launch_bounds__(TH) void k_app(const uint16_t* __restrict__ frames, int NF, int H, int W,
                                            const int* __restrict__ fmeta, const int* __restrict__ fcount,
                                            const int* __restrict__ pix, long long NP, const int* __restrict__ ameta,
                                            const int* __restrict__ idx, uint32_t k0, uint32_t k1, uint32_t res,
                                            const uint32_t* __restrict__ crc, const double* __restrict__ cmin,
                                            const int* __restrict__ cgrid, int B, long long NV, double voxel,
                                            const int* __restrict__ vol0f, const double* __restrict__ norm,
                                            double* __restrict__ out, int* __restrict__ err) {
    const int a = blockIdx.x, t = threadIdx.x;
    const int g = ameta[a * 3], b = ameta[a * 3 + 1], slot = ameta[a * 3 + 2];
    if (g < 0 || g >= NF || b < 0 || b >= B) { if (t == 0) atomicOr(err, E_BIT); return; }
    const int cnt = fcount[g], poff = fmeta[g * 4 + 3];
    if (cnt <= 0 || poff < 0 || (long long)poff + cnt > NP) { if (t == 0) atomicOr(err, E_EMPTY); return; }
    const uint16_t* im = frames + (size_t)g * H * W;
    const double m[3] = {cmin[b * 3], cmin[b * 3 + 1], cmin[b * 3 + 2]};
    const int nx = cgrid[b * 4], ny = cgrid[b * 4 + 1], nz = cgrid[b * 4 + 2];
    const long long base = cgrid[b * 4 + 3];
    const double* nb = norm + b * NORM;
    const double ylen = nb[3], c0 = nb[4], l0 = nb[9];
    for (int h = 0; h < 2; ++h) {
        const int n = t + h * TH;
        int i;
        if (idx) {
            i = idx[(size_t)a * NS + n];
        } else if (cnt < NS && n < cnt) {
            i = n;
        } else {
            i = draw_row(philox4x32_10((uint32_t)n, (uint32_t)(2 + slot), crc[b], res, k0, k1).w[0], cnt);
        }
        if (i < 0 || i >= cnt) { atomicOr(err, E_INDEX); i = 0; }
        int p = pix[poff + i];
        if (p < 0 || p >= H * W) { atomicOr(err, E_PIXEL); p = 0; }
        const int r = p / W, c = p - r * W;
        double P[3];
        backproject(r, c, (int)im[p], P[0], P[1], P[2]);
        double v[3];
        int iv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[k] = (P[k] - m[k]) / voxel; iv[k] = (int)v[k]; }
        const long long q = base + ((long long)iv[0] * ny + iv[1]) * nz + iv[2];
        int mot = 0;
        if (iv[0] < 0 || iv[0] >= nx || iv[1] < 0 || iv[1] >= ny || iv[2] < 0 || iv[2] >= nz || q >= NV)
            atomicOr(err, E_VOXEL);
        else
            mot = vol0f[q];
        double* o = out + ((size_t)a * NS + n) * 4;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (v[k] - nb[k]) / ylen;
        o[3] = ((double)mot - c0) / l0 - 0.5;
    }
}

inline bool bad_image(int NF, int H, int W) {
    return NF < 1 || NF > FACL_GEN3DV_MAX_FRAMES_TOTAL || H < 1 || W < 1 || (long long)H * W > FACL_GEN3DV_MAX_PIXELS;
}
inline bool bad_grid(int B, int maxvox, int64_t NV) {
    return B < 1 || B > FACL_GEN3DV_MAX_CLIPS || maxvox < 1 || maxvox > FACL_GEN3DV_MAX_VOXELS || NV < maxvox ||
           NV > FACL_GEN3DV_MAX_VOXELS_TOTAL;
}

}  // namespace

extern "C" int facl_gen3dv_frames(const uint16_t* frames, int NF, int H, int W, int32_t* fbox, int32_t* fcount,
                                  double* fext, void* stream) {
    if (!frames || !fbox || !fcount || !fext) return FACL_E_NULL;
    if (bad_image(NF, H, W)) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_frames, dim3(NF), dim3(TH), 0, (hipStream_t)stream, frames, H, W, fbox, fcount, fext);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_voxelise(const uint16_t* frames, int NF, int H, int W, const int32_t* fbox,
                                    const int32_t* fmeta, const double* cmin, const int32_t* cgrid, int B, int maxF,
                                    int maxvox, int64_t NV, int64_t NP, double voxel, uint64_t* occ, uint64_t* mocc,
                                    int32_t* pix, int32_t* err, void* stream) {
    if (!frames || !fbox || !fmeta || !cmin || !cgrid || !occ || !mocc || !pix || !err) return FACL_E_NULL;
    if (bad_image(NF, H, W) || bad_grid(B, maxvox, NV) || maxF < 1 || maxF > FACL_GEN3DV_MAX_FRAMES || NP < 1 ||
        NP > (int64_t)NF * H * W || NP > INT32_MAX || !(voxel > 0.0))
        return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_voxelise, dim3(NF), dim3(TH), 0, (hipStream_t)stream, frames, NF, H, W, fbox, fmeta, cmin, cgrid,
                       B, maxF, (long long)NV, (long long)NP, voxel, (unsigned long long*)occ, (unsigned long long*)mocc,
                       pix, err);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_volumes(const uint64_t* occ, const uint64_t* mocc, const int32_t* wtab, const int32_t* cgrid,
                                   int B, int maxvox, int64_t NV, int32_t* vol, int32_t* key, void* stream) {
    if (!occ || !mocc || !wtab || !cgrid || !vol || !key) return FACL_E_NULL;
    if (bad_grid(B, maxvox, NV)) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_volumes, dim3((maxvox + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)occ, (const unsigned long long*)mocc, wtab, cgrid, (long long)NV, vol,
                       key);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_filter(const int32_t* vol, const int32_t* key, const int32_t* cgrid, int B, int maxvox,
                                  int64_t NV, int th_all, int th_key, int32_t* vol0f, int32_t* keyf, void* stream) {
    if (!vol || !key || !cgrid || !vol0f || !keyf) return FACL_E_NULL;
    if (bad_grid(B, maxvox, NV) || th_all < 2 || th_all > 27 || th_key < 2 || th_key > 27) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_filter, dim3((maxvox + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, vol, key, cgrid,
                       (long long)NV, th_all, th_key, vol0f, keyf);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_compact(const int32_t* vol, const int32_t* vol0f, const int32_t* keyf, const int32_t* cgrid,
                                   int B, int maxvox, int64_t NV, int32_t* lists, int32_t* counts, void* stream) {
    if (!vol || !vol0f || !keyf || !cgrid || !lists || !counts) return FACL_E_NULL;
    if (bad_grid(B, maxvox, NV)) return FACL_E_SHAPE;
    hipLaunchKernelGGL(k_compact, dim3(4, B), dim3(TH), 0, (hipStream_t)stream, vol, vol0f, keyf, cgrid, (long long)NV,
                       lists, counts);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_sample(const int32_t* vol, const int32_t* vol0f, const int32_t* lists, const int32_t* counts,
                                  const int32_t* cgrid, int B, int maxvox, int64_t NV, const int32_t* idx, int64_t seed,
                                  int resolution, const uint32_t* crc, double* out_raw, double* out_key, double* norm,
                                  int32_t* err, void* stream) {
    if (!vol || !vol0f || !lists || !counts || !cgrid || !out_raw || !out_key || !norm || !err || (!idx && !crc))
        return FACL_E_NULL;
    if (bad_grid(B, maxvox, NV)) return FACL_E_SHAPE;
    const uint64_t s = (uint64_t)seed;
    hipLaunchKernelGGL(k_sample, dim3(B), dim3(TH), 0, (hipStream_t)stream, vol, vol0f, lists, counts, cgrid,
                       (long long)NV, idx, (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), (uint32_t)resolution, crc,
                       out_raw, out_key, norm, err);
    return facl_launch_status();
}

extern "C" int facl_gen3dv_app(const uint16_t* frames, int NF, int H, int W, const int32_t* fmeta, const int32_t* fcount,
                               const int32_t* pix, int64_t NP, const int32_t* ameta, int NA, const int32_t* idx,
                               int64_t seed, int resolution, const uint32_t* crc, const double* cmin,
                               const int32_t* cgrid, int B, int maxvox, int64_t NV, double voxel, const int32_t* vol0f,
                               const double* norm, double* out, int32_t* err, void* stream) {
    if (!frames || !fmeta || !fcount || !pix || !ameta || !cmin || !cgrid || !vol0f || !norm || !out || !err ||
        (!idx && !crc))
        return FACL_E_NULL;
    if (bad_image(NF, H, W) || bad_grid(B, maxvox, NV) || NA < 1 || NA > FACL_GEN3DV_MAX_FRAMES_TOTAL || NP < 1 ||
        NP > INT32_MAX || !(voxel > 0.0))
        return FACL_E_SHAPE;
    const uint64_t s = (uint64_t)seed;
    hipLaunchKernelGGL(k_app, dim3(NA), dim3(TH), 0, (hipStream_t)stream, frames, NF, H, W, fmeta, fcount, pix,
                       (long long)NP, ameta, idx, (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), (uint32_t)resolution,
                       crc, cmin, cgrid, B, (long long)NV, voxel, vol0f, norm, out, err);
    return facl_launch_status();
}
