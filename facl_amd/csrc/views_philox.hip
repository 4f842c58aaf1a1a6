// The views of a batch of clips with COUNTER-BASED draws (--view_rng philox): no host draw per clip, no host mask
// loop, two launches per batch.  G views of P points per clip; G = 10, P = 512 is the reference's loader.  Same views
// as csrc/views.hip (cn3D_data_set.py:285-350 get_data_train, :654-663, :708-713, :734-749, :767-778) and the same arithmetic -- only the random numbers come from Philox4x32-10 instead of
// NumPy's stream, so a clip's views depend on (seed, epoch, dataset index of the clip) and on nothing else: not on its
// position in the batch, the batch size or the number of ranks.
//
// Draw recipe (restated in NumPy by facl_amd/philox.py, which the tests hold this file to), written for the first ten
// views ("views 0..9" below are the ten KINDS: raw, reversed, key, key-reversed, rotated x2, temporal channel 4, temporal
// channel 7, low-res x2):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (point n in 0..P-1, slot, clip id, epoch)           -> four 32-bit words w0..w3
//   rows    slot 0: views 0,1,2,3 = w0..w3; slot 1: views 4,5,6,7; slot 2: views 8,9 = w0,w1.
//           row = (uint64(w) * count) >> 32 in [0, count) of the view's source cloud (views 6, 7: of the list of rows
//           whose channel 4 / 7 is non-zero, compacted by k_temporal_rows)
//   jitter  slot 3 + 3*j + d (j = jitter slot 0..6 of views.hip, d = xyz): u1 = (w0 + 1) * 2^-32 in (0, 1],
//           u2 = w1 * 2^-32 in [0, 1), z = sqrt(-2 log u1) * cos(2 pi u2) in fp64, then clip(0.01 z, -0.05, 0.05)
//   angle k (k = 0, 1; views 4, 5): counter (0, 24 + k, clip id, epoch), u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53,
//           angle = (u - 0.5) * pi * 0.8, cos / sin in fp64
// Any G and P (the reference has no recipe beyond 10 x 512: an extension, on this stream only):
//   view v  is of kind k = v % 10 in round r = v / 10 and draws as kind k does, with EVERY slot moved by 32 * r: its row
//           word is word k & 3 of slot (k >> 2) + 32 r, its jitter slots are 3 + 3 j + d + 32 r, its angle slot 24 + (k - 4)
//           + 32 r.  Slots 0..25 of a round are in use, so rounds never share a counter.
//   point n runs over 0..P-1 in counter word 0; nothing else changes.
//   domain  1 <= G <= 64; 64 <= P <= 4096 with P % 64 == 0 (the grouping limit); FACL_E_SHAPE otherwise.
// So a view's values do not depend on G, its first P' points do not depend on P, and G = 10, P = 512 -- the entries
// without _gp, which call the same launcher -- is the block [v < 10, n < 512] of every other size, bit for bit.
// Arithmetic: k_build_views' dtype walk -- jitter in fp64 written back in the source dtype, mirror / rotation on float32.
#include "common.h"

namespace {

#include "views_philox_point.inc"         // the Philox block, the draw recipe and the per-point arithmetic (shared with
                                          // views_resident.hip, whose views must equal these bit for bit)

// meta (B, 9) int32 per clip: row offset of the four source clouds in src, their row counts, the clip's dataset index
constexpr int META = 9;

// one workgroup per clip: the rows of its point cloud whose channel 4 / channel 7 is non-zero, in row order, written to
// list[0][base0 + k] / list[1][base0 + k] (k < count); counts (B, 2).  A zero count raises err (the views must not be used).
template <typename S>
__global__ __launch_bounds__(TR_THREADS) void k_temporal_rows(const S* __restrict__ src, int C, int rows,
                                                              const int* __restrict__ meta, int* __restrict__ list,
                                                              int* __restrict__ counts, int* __restrict__ err) {
    __shared__ int wtot[2][TR_THREADS / FACL_WAVE];
    const int b = blockIdx.x;
    const int base = meta[b * META], P = meta[b * META + 4];
    int run4 = 0, run7 = 0;                                       // rows kept so far (uniform across the block)
    for (int c = 0; c < P; c += TR_THREADS)
        temporal_rows_pass<S, int>(src + (size_t)base * C, C, P, c, base, list + base, list + (size_t)rows + base, run4,
                                   run7, wtot);
    if (threadIdx.x == 0) {
        counts[b * 2] = run4;
        counts[b * 2 + 1] = run7;
        if (run4 == 0 || run7 == 0) *err = 1;
    }
}

// workgroup = one (clip, view, chunk of up to 512 points); thread = one point.  idx_out (B, G, P), optional: the absolute
// source row of every point.
template <typename S>
__global__ __launch_bounds__(CHUNK) void k_build_views_philox(const S* __restrict__ src, int C, int rows,
                                                              const int* __restrict__ meta, const int* __restrict__ list,
                                                              const int* __restrict__ counts, int64_t seed, int epoch, int B,
                                                              int G, int P, int chunks, float* __restrict__ out,
                                                              int* __restrict__ idx_out) {
    const ViewAt at = view_at(G, chunks);
    const int b = at.b, k = at.k, n = at.n;
    if (n >= P) return;                                          // the ragged last chunk of a view
    const int* m = meta + b * META;
    const ViewDraw q = view_draw(seed, (uint32_t)m[8], epoch);
    float* dst = out + (((size_t)at.v * B + b) * P + n) * 4;
    int* io = idx_out ? idx_out + ((size_t)b * G + at.v) * P + n : nullptr;
    const int src_of = view_source(k);
    const uint32_t word = view_row_word(q, k, at.slot0, n);
    int row;
    if (k == 6 || k == 7) {
        const int cnt = counts[b * 2 + (k - 6)];
        if (cnt == 0) {                                          // no row to draw from: err is set, the views are void
            view_void(dst);
            if (io) *io = -1;
            return;
        }
        row = list[(size_t)(k - 6) * rows + m[0] + draw_row(word, cnt)];
    } else {
        row = m[src_of] + draw_row(word, m[4 + src_of]);
    }
    if (io) *io = row;
    view_point<S>(src + (size_t)row * C, q, k, at.slot0, n, dst);
}

}  // namespace

template <typename S>
static int launch_temporal_rows(const S* src, int64_t rows, int C, const int32_t* meta, int B, int32_t* list,
                                int32_t* counts, int32_t* err, void* stream) {
    if (!src || !meta || !list || !counts || !err) return FACL_E_NULL;
    if (B < 1 || rows < 1 || rows > INT32_MAX / 2 || C < 8 || B > (1 << 20)) return FACL_E_SHAPE;
    hipLaunchKernelGGL((k_temporal_rows<S>), dim3(B), dim3(TR_THREADS), 0, (hipStream_t)stream, src, C, (int)rows, meta,
                       list, counts, err);
    return facl_launch_status();
}

template <typename S>
static int launch_views_philox(const S* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                               const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                               int32_t* idx_out, void* stream) {
    if (!src || !meta || !list || !counts || !out) return FACL_E_NULL;
    if (B < 1 || rows < 1 || rows > INT32_MAX / 2 || C < 8 || B > (1 << 20) || !views_gp_ok(G, P)) return FACL_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) % 16) return FACL_E_ALIGN;
    const ViewGrid g = view_grid(P);
    hipLaunchKernelGGL((k_build_views_philox<S>), dim3((unsigned)B * G * g.chunks), dim3(g.threads), 0, (hipStream_t)stream,
                       src, C, (int)rows, meta, list, counts, seed, epoch, B, G, P, g.chunks, out, idx_out);
    return facl_launch_status();
}

extern "C" int facl_views_temporal_rows_f32(const float* src, int64_t rows, int C, const int32_t* meta, int B,
                                            int32_t* list, int32_t* counts, int32_t* err, void* stream) {
    return launch_temporal_rows<float>(src, rows, C, meta, B, list, counts, err, stream);
}

extern "C" int facl_views_temporal_rows_f64(const double* src, int64_t rows, int C, const int32_t* meta, int B,
                                            int32_t* list, int32_t* counts, int32_t* err, void* stream) {
    return launch_temporal_rows<double>(src, rows, C, meta, B, list, counts, err, stream);
}

extern "C" int facl_build_views_philox_f32(const float* src, int64_t rows, int C, const int32_t* meta,
                                           const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                           float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, KINDS, CHUNK, out, idx_out, stream);
}

extern "C" int facl_build_views_philox_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                           const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                           float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, KINDS, CHUNK, out, idx_out, stream);
}

extern "C" int facl_build_views_philox_gp_f32(const float* src, int64_t rows, int C, const int32_t* meta,
                                              const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                              int G, int P, float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, stream);
}

extern "C" int facl_build_views_philox_gp_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                              const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                              int G, int P, float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, stream);
}
