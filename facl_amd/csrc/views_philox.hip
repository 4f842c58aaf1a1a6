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
// Any RECIPE (a list of L = 1..12 kinds, the positions of a round, and six strengths; the text above is the default one):
//   view v  is of the kind at position v % L in round v / L; every slot of round r is the position's slot + stride * r.
//   kinds   raw, mirror, key, key_mirror, rot, t4, t7, res30, res10 (above); jitter = points, jitter; scale = points, jitter,
//           xyz * s; tilt_neg / tilt_pos = points, jitter, rotation about y by -/+ pi * tilt_angle (cn3D_data_set.py:356-358,
//           :697-704 then :757-763 / :716-732)
//   slots   row word of position i: word i & 3 of slot i >> 2.  Jitter draws are numbered j = 0, 1, ... in position order
//           (mirror, key_mirror: two; key, rot, jitter, scale, tilt_*: one) and draw j uses slots 3 + 3 j + d.  Scalar draws (rot,
//           scale: one each) are numbered in position order from 3 + 3 max(7, J), J = jitter draws of the round.  stride =
//           32 ceil((3 + 3 max(7, J) + A) / 32), A = scalar draws.  The default list gives the layout above (j = 0..6, scalars
//           24, 25, stride 32).  So a view's draws depend on the kinds BEFORE it in the list.
//   dtype walk (S = source dtype):
//     jitter  before any float32 operation: x = S(double(x) + clip(jitter_sigma * z, +-jitter_clip)), jit()'s evaluation
//             order (0.01 / 0.05 give the earlier bits); the second jitter of the mirrored kinds on float32
//     rot     on double(float(x)): fx c + fz (-s), fy, fx s + fz c, rounded to float32; angle = ((u - 0.5) * pi) * rot_range
//     tilt_*  the same rotation with cos / sin of pi * tilt_angle, computed once on the host and passed by value
//     scale   s = scale_lo + (scale_hi - scale_lo) * u in fp64 as written (contraction off), rounded to S; the product in S,
//             cast to float32 (NumPy with a Python-float factor and an S array); u = uniform53 of the position's scalar slot
//   The descriptors and strengths travel BY VALUE in the kernel arguments; REF = true is the default recipe folded into the code.
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
// source row of every point.  REF: the default recipe folded into the code (views_philox_point.inc); rc is then unread.
template <typename S, bool REF>
__global__ __launch_bounds__(CHUNK) void k_build_views_philox(const S* __restrict__ src, int C, int rows,
                                                              const int* __restrict__ meta, const int* __restrict__ list,
                                                              const int* __restrict__ counts, int64_t seed, int epoch, int B,
                                                              int G, int P, int chunks, float* __restrict__ out,
                                                              int* __restrict__ idx_out, const ViewRecipe rc) {
    const ViewAt at = REF ? view_at_reference(G, chunks) : view_at(rc, G, chunks);
    const int b = at.b, n = at.n;
    if (n >= P) return;                                          // the ragged last chunk of a view
    const ViewPos d = REF ? ViewPos{} : rc.pos[at.k];
    const int* m = meta + b * META;
    const ViewDraw q = view_draw(seed, (uint32_t)m[8], epoch);
    float* dst = out + (((size_t)at.v * B + b) * P + n) * 4;
    int* io = idx_out ? idx_out + ((size_t)b * G + at.v) * P + n : nullptr;
    const int src_of = REF ? view_source_reference(at.k) : (int)d.src;
    const uint32_t word = REF ? view_row_word_reference(q, at.k, at.slot0, n) : view_row_word(q, d, at.slot0, n);
    int row;
    if (src_of >= SRC_T4) {
        const int t = src_of - SRC_T4;
        const int cnt = counts[b * 2 + t];
        if (cnt == 0) {                                          // no row to draw from: err is set, the views are void
            view_void(dst);
            if (io) *io = -1;
            return;
        }
        row = list[(size_t)t * rows + m[0] + draw_row(word, cnt)];
    } else {
        row = m[src_of] + draw_row(word, m[4 + src_of]);
    }
    if (io) *io = row;
    if (REF) view_point_reference<S>(src + (size_t)row * C, q, at.k, at.slot0, n, dst);
    else view_point<S>(src + (size_t)row * C, q, rc, d, at.slot0, n, dst);
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
                               int32_t* idx_out, const ViewRecipe& rc, void* stream) {
    if (!src || !meta || !list || !counts || !out) return FACL_E_NULL;
    if (B < 1 || rows < 1 || rows > INT32_MAX / 2 || C < 8 || B > (1 << 20) || !views_gp_ok(G, P)) return FACL_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) % 16) return FACL_E_ALIGN;
    const ViewGrid g = view_grid(P);
    const auto kernel = view_recipe_is_default(rc) ? k_build_views_philox<S, true> : k_build_views_philox<S, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B * G * g.chunks), dim3(g.threads), 0, (hipStream_t)stream, src, C, (int)rows,
                       meta, list, counts, seed, epoch, B, G, P, g.chunks, out, idx_out, rc);
    return facl_launch_status();
}

// the recipe entries: the caller's HOST arrays are checked and turned into the recipe first (no launch on a refusal)
template <typename S>
static int launch_views_philox_recipe(const S* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                      const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                                      int32_t* idx_out, const int32_t* kinds, int n_kinds, const double* strengths,
                                      void* stream) {
    ViewRecipe rc;
    const int e = view_recipe_make(kinds, n_kinds, strengths, &rc);
    if (e != 0) return e;
    return launch_views_philox<S>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, rc, stream);
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
    return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, KINDS, CHUNK, out, idx_out, view_recipe_default(),
                                      stream);
}

extern "C" int facl_build_views_philox_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                           const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                           float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, KINDS, CHUNK, out, idx_out, view_recipe_default(),
                                      stream);
}

extern "C" int facl_build_views_philox_gp_f32(const float* src, int64_t rows, int C, const int32_t* meta,
                                              const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                              int G, int P, float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, view_recipe_default(), stream);
}

extern "C" int facl_build_views_philox_gp_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                              const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                              int G, int P, float* out, int32_t* idx_out, void* stream) {
    return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, view_recipe_default(), stream);
}

extern "C" int facl_build_views_philox_recipe_f32(const float* src, int64_t rows, int C, const int32_t* meta,
                                                  const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                                  int G, int P, float* out, int32_t* idx_out, const int32_t* kinds,
                                                  int n_kinds, const double* strengths, void* stream) {
    return launch_views_philox_recipe<float>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, kinds,
                                             n_kinds, strengths, stream);
}

extern "C" int facl_build_views_philox_recipe_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                                  const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                                  int G, int P, float* out, int32_t* idx_out, const int32_t* kinds,
                                                  int n_kinds, const double* strengths, void* stream) {
    return launch_views_philox_recipe<double>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, kinds,
                                              n_kinds, strengths, stream);
}

extern "C" int facl_view_recipe_table(const int32_t* kinds, int n_kinds, int32_t* table, int32_t* stride) {
    return view_recipe_table(kinds, n_kinds, table, stride);
}
