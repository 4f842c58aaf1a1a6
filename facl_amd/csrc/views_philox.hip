// The views of a batch of clips with COUNTER-BASED draws (--view_rng philox): no host draw per clip, no host mask
// loop, two launches per batch.  G views of P points per clip; G = 10, P = 512 is the reference's loader.  Same views
// as csrc/views.hip (cn3D_data_set.py:285-350 get_data_train, :654-663, :708-713, :734-749, :767-778) and the same arithmetic -- only the random numbers come from Philox4x32-10 instead of
// NumPy's stream, so a clip's views depend on (seed, epoch, dataset index of the clip) and on nothing else: not on its
// position in the batch, the batch size or the number of ranks.
//
// The draw recipe, the domain of (G, P), the view recipes and the dtype walk are written out in csrc/views_point.inc, which
// holds the draws, the arithmetic, the kernel body and the launcher tail shared with views_resident.hip (whose views must
// equal these bit for bit).  Particular to this file: the batch arrives PACKED (facl_amd/views.py: pack_clips), the rows of
// the temporal views are compacted per batch (k_temporal_rows), and source rows are int32.
#include "common.h"

namespace {

#include "views_point.inc"

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

// how a drawn position becomes a row of the packed batch (build_view's `from`): through the clip's meta record
struct FromBatch {
    const int *meta, *list, *counts;
    int rows, C;
    const int* m;                                                // the clip's meta record, set by clip()
    int b;
    __device__ bool clip(int b_, bool) { b = b_; m = meta + b * META; return true; }
    __device__ uint32_t cid() const { return (uint32_t)m[8]; }
    __device__ int temporal_count(int t) const { return counts[b * 2 + t]; }
    __device__ int temporal_row(int t, int k) const { return list[(size_t)t * rows + m[0] + k]; }
    __device__ int cloud_row(int s, uint32_t word) const { return m[s] + draw_row(word, m[4 + s]); }
    __device__ size_t channels() const { return (size_t)C; }
};

// build_view on a packed batch.  idx_out (B, G, P), optional: the absolute source row of every point.
template <typename S, bool REF>
__global__ __launch_bounds__(CHUNK) void k_build_views_philox(const S* __restrict__ src, int C, int rows,
                                                              const int* __restrict__ meta, const int* __restrict__ list,
                                                              const int* __restrict__ counts, int64_t seed, int epoch, int B,
                                                              int G, int P, int chunks, float* __restrict__ out,
                                                              int* __restrict__ idx_out, const ViewRecipe rc) {
    build_view<S, REF>(src, FromBatch{meta, list, counts, rows, C, nullptr, 0}, B, G, P, chunks, seed, epoch, out, idx_out, rc);
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
    const int own = (!src || !meta || !list || !counts || !out) ? FACL_E_NULL
                    : (rows < 1 || rows > INT32_MAX / 2 || C < 8) ? FACL_E_SHAPE : 0;
    return view_launch(own, k_build_views_philox<S, true>, k_build_views_philox<S, false>, B, G, P, out, rc,
                       [&](auto kernel, dim3 grid, dim3 threads, int chunks) {
                           hipLaunchKernelGGL(kernel, grid, threads, 0, (hipStream_t)stream, src, C, (int)rows, meta, list,
                                              counts, seed, epoch, B, G, P, chunks, out, idx_out, rc);
                       });
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
    return with_view_recipe(kinds, n_kinds, strengths, [&](const ViewRecipe& rc) {
        return launch_views_philox<float>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, rc, stream);
    });
}

extern "C" int facl_build_views_philox_recipe_f64(const double* src, int64_t rows, int C, const int32_t* meta,
                                                  const int32_t* list, const int32_t* counts, int64_t seed, int epoch, int B,
                                                  int G, int P, float* out, int32_t* idx_out, const int32_t* kinds,
                                                  int n_kinds, const double* strengths, void* stream) {
    return with_view_recipe(kinds, n_kinds, strengths, [&](const ViewRecipe& rc) {
        return launch_views_philox<double>(src, rows, C, meta, list, counts, seed, epoch, B, G, P, out, idx_out, rc, stream);
    });
}

extern "C" int facl_view_recipe_table(const int32_t* kinds, int n_kinds, int32_t* table, int32_t* stride) {
    return view_recipe_table(kinds, n_kinds, table, stride);
}
