// The philox views of clips that are RESIDENT in device memory (--resident 1): the whole training split is loaded once
// into a pool, and a batch is B table positions.  No file is read, nothing is packed and no clip data crosses to the
// device per step.  The views equal csrc/views_philox.hip's bit for bit: the draws, the per-point arithmetic and the kernel
// body are the same code (views_point.inc, where the recipe is written out); only the way a drawn position becomes a source
// row differs (FromPool), and source rows are int64.
//
// Pool (device memory owned by facl_amd/resident.py):
//   src    (rows_total, 8) in the dataset's one dtype: the clips back to back, each as its four clouds in pack_clips' order
//   table  (n_clips, FACL_RESIDENT_REC) int64, one record per clip:
//            [0..3]  row offset in src of points, key points, res1, res2 (64-bit: an NTU-120 split is over 6e8 rows)
//            [4..7]  their row counts (>= 1; a clip's rows together < 2^31)
//            [8]     dataset index of the clip = the philox counter word `cid`
//            [9]     L = sum of the point-cloud rows of the clips before it: the clip's slot in `lists`
//            [10,11] number of rows of its point cloud whose channel 4 / channel 7 is non-zero (written by the ingest pass)
//   lists  (2 * sum of point-cloud rows) int32: for the clip at slot L with P point-cloud rows, lists[2L .. 2L + n4) are
//          the rows with a non-zero channel 4 and lists[2L + P .. 2L + P + n7) those with a non-zero channel 7, in row
//          order, RELATIVE to the clip's first row.  They depend on the data only: built once at ingest.
//   err    (2) int32: [0] flags, only ever raised: 1 = a clip without temporal rows, 2 = a selection outside the table;
//          [1] = the smallest table position with flag 1 (the caller initialises it to INT32_MAX).
#include "common.h"

namespace {

#include "views_point.inc"

constexpr int REC = FACL_RESIDENT_REC, RC = 8;      // int64 words per table record; channels per pool row

// ingest: one workgroup per table record first + blockIdx.x
template <typename S>
__global__ __launch_bounds__(TR_THREADS) void k_resident_temporal_rows(const S* __restrict__ src,
                                                                       int64_t* __restrict__ table,
                                                                       int32_t* __restrict__ lists, int first,
                                                                       int32_t* __restrict__ err) {
    __shared__ int wtot[2][TR_THREADS / FACL_WAVE];
    const int pos = first + (int)blockIdx.x;
    int64_t* rec = table + (int64_t)pos * REC;
    const int64_t base = rec[0], L = rec[9];
    const int P = (int)rec[4];
    int32_t* l4 = lists + 2 * L;
    int run4 = 0, run7 = 0;
    for (int c = 0; c < P; c += TR_THREADS)
        temporal_rows_pass<S, int32_t>(src + base * RC, RC, P, c, 0, l4, l4 + P, run4, run7, wtot);
    if (threadIdx.x == 0) {
        rec[10] = run4;
        rec[11] = run7;
        if (run4 == 0 || run7 == 0) {
            atomicOr(err, 1);
            atomicMin(err + 1, pos);
        }
    }
}

// how a drawn position becomes a row of the pool (build_view's `from`): through the table record of the selected clip
struct FromPool {
    const int64_t* table;
    const int32_t *lists, *sel;
    int n_clips;
    int32_t* err;
    const int64_t* m;                                              // the clip's table record, set by clip()
    __device__ bool clip(int b, bool first) {
        const int pos = sel[b];
        if (pos < 0 || pos >= n_clips) {                           // not a clip of the pool: no pool memory is touched
            if (first) atomicOr(err, 2);
            return false;
        }
        m = table + (int64_t)pos * REC;
        return true;
    }
    __device__ uint32_t cid() const { return (uint32_t)m[8]; }
    __device__ int temporal_count(int t) const { return (int)m[10 + t]; }      // 0: the ingest raised err for this clip
    __device__ int64_t temporal_row(int t, int k) const { return m[0] + lists[2 * m[9] + t * m[4] + k]; }
    __device__ int64_t cloud_row(int s, uint32_t word) const { return m[s] + draw_row(word, (int)m[4 + s]); }
    __device__ int64_t channels() const { return RC; }
};

// build_view on the pool.  idx_out (B, G, P) int64, optional: the pool row of every point.
template <typename S, bool REF>
__global__ __launch_bounds__(CHUNK) void k_build_views_resident(const S* __restrict__ src, const int64_t* __restrict__ table,
                                                                const int32_t* __restrict__ lists, int n_clips,
                                                                const int32_t* __restrict__ sel, int B, int G, int P,
                                                                int chunks, int64_t seed, int epoch, float* __restrict__ out,
                                                                int64_t* __restrict__ idx_out, int32_t* __restrict__ err,
                                                                const ViewRecipe rc) {
    build_view<S, REF>(src, FromPool{table, lists, sel, n_clips, err, nullptr}, B, G, P, chunks, seed, epoch, out, idx_out, rc);
}

}  // namespace

template <typename S>
static int launch_resident_rows(const S* src, int64_t* table, int32_t* lists, int first, int count, int32_t* err,
                                void* stream) {
    if (!src || !table || !lists || !err) return FACL_E_NULL;
    if (first < 0 || count < 1 || (int64_t)first + count > INT32_MAX) return FACL_E_SHAPE;
    hipLaunchKernelGGL((k_resident_temporal_rows<S>), dim3(count), dim3(TR_THREADS), 0, (hipStream_t)stream, src, table,
                       lists, first, err);
    return facl_launch_status();
}

template <typename S>
static int launch_views_resident(const S* src, const int64_t* table, const int32_t* lists, int n_clips, const int32_t* sel,
                                 int B, int G, int P, int64_t seed, int epoch, float* out, int64_t* idx_out, int32_t* err,
                                 const ViewRecipe& rc, void* stream) {
    const int own = (!src || !table || !lists || !sel || !out || !err) ? FACL_E_NULL : n_clips < 1 ? FACL_E_SHAPE : 0;
    return view_launch(own, k_build_views_resident<S, true>, k_build_views_resident<S, false>, B, G, P, out, rc,
                       [&](auto kernel, dim3 grid, dim3 threads, int chunks) {
                           hipLaunchKernelGGL(kernel, grid, threads, 0, (hipStream_t)stream, src, table, lists, n_clips, sel,
                                              B, G, P, chunks, seed, epoch, out, idx_out, err, rc);
                       });
}

extern "C" int facl_resident_temporal_rows_f32(const float* src, int64_t* table, int32_t* lists, int first, int count,
                                               int32_t* err, void* stream) {
    return launch_resident_rows<float>(src, table, lists, first, count, err, stream);
}

extern "C" int facl_resident_temporal_rows_f64(const double* src, int64_t* table, int32_t* lists, int first, int count,
                                               int32_t* err, void* stream) {
    return launch_resident_rows<double>(src, table, lists, first, count, err, stream);
}

extern "C" int facl_build_views_resident_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                             const int32_t* sel, int B, int64_t seed, int epoch, float* out,
                                             int64_t* idx_out, int32_t* err, void* stream) {
    return launch_views_resident<float>(src, table, lists, n_clips, sel, B, KINDS, CHUNK, seed, epoch, out, idx_out, err,
                                        view_recipe_default(), stream);
}

extern "C" int facl_build_views_resident_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                             const int32_t* sel, int B, int64_t seed, int epoch, float* out,
                                             int64_t* idx_out, int32_t* err, void* stream) {
    return launch_views_resident<double>(src, table, lists, n_clips, sel, B, KINDS, CHUNK, seed, epoch, out, idx_out, err,
                                        view_recipe_default(), stream);
}

extern "C" int facl_build_views_resident_gp_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                                const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                                int64_t* idx_out, int32_t* err, void* stream) {
    return launch_views_resident<float>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err,
                                        view_recipe_default(), stream);
}

extern "C" int facl_build_views_resident_gp_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                                const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                                int64_t* idx_out, int32_t* err, void* stream) {
    return launch_views_resident<double>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err,
                                        view_recipe_default(), stream);
}

extern "C" int facl_build_views_resident_recipe_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                                    const int32_t* sel, int B, int G, int P, int64_t seed, int epoch,
                                                    float* out, int64_t* idx_out, int32_t* err, const int32_t* kinds,
                                                    int n_kinds, const double* strengths, void* stream) {
    return with_view_recipe(kinds, n_kinds, strengths, [&](const ViewRecipe& rc) {
        return launch_views_resident<float>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err, rc, stream);
    });
}

extern "C" int facl_build_views_resident_recipe_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                                    const int32_t* sel, int B, int G, int P, int64_t seed, int epoch,
                                                    float* out, int64_t* idx_out, int32_t* err, const int32_t* kinds,
                                                    int n_kinds, const double* strengths, void* stream) {
    return with_view_recipe(kinds, n_kinds, strengths, [&](const ViewRecipe& rc) {
        return launch_views_resident<double>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err, rc, stream);
    });
}
