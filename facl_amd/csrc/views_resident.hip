// The philox views of clips that are RESIDENT in device memory (--resident 1): the whole training split is loaded once
// into a pool, and a batch is B table positions.  No file is read, nothing is packed and no clip data crosses to the
// device per step.  The views equal csrc/views_philox.hip's bit for bit: the draw recipe and the per-point arithmetic are
// the same code (views_philox_point.inc); only the way a drawn position becomes a source row differs.  G views of P
// points per clip, by the recipe in the header of views_philox.hip (default: kind v % 10, round v / 10, slots + 32 * round;
// any other list of kinds and strengths through the same ViewRecipe, passed by value).
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

#include "views_philox_point.inc"

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

// workgroup = one (clip of the batch, view, chunk of up to 512 points); thread = one point.  idx_out (B, G, P) int64,
// optional: the pool row of every point.  REF: the default recipe folded into the code (views_philox_point.inc).
template <typename S, bool REF>
__global__ __launch_bounds__(CHUNK) void k_build_views_resident(const S* __restrict__ src, const int64_t* __restrict__ table,
                                                                const int32_t* __restrict__ lists, int n_clips,
                                                                const int32_t* __restrict__ sel, int B, int G, int P,
                                                                int chunks, int64_t seed, int epoch, float* __restrict__ out,
                                                                int64_t* __restrict__ idx_out, int32_t* __restrict__ err,
                                                                const ViewRecipe rc) {
    const ViewAt at = REF ? view_at_reference(G, chunks) : view_at(rc, G, chunks);
    const int b = at.b, n = at.n;
    if (n >= P) return;                                            // the ragged last chunk of a view
    float* dst = out + (((size_t)at.v * B + b) * P + n) * 4;
    int64_t* io = idx_out ? idx_out + ((size_t)b * G + at.v) * P + n : nullptr;
    const int pos = sel[b];
    if (pos < 0 || pos >= n_clips) {                               // not a clip of the pool: no pool memory is touched
        if (n == 0 && at.v == 0) atomicOr(err, 2);
        view_void(dst);
        if (io) *io = -1;
        return;
    }
    const ViewPos d = REF ? ViewPos{} : rc.pos[at.k];
    const int64_t* m = table + (int64_t)pos * REC;
    const ViewDraw q = view_draw(seed, (uint32_t)m[8], epoch);
    const int src_of = REF ? view_source_reference(at.k) : (int)d.src;
    const uint32_t word = REF ? view_row_word_reference(q, at.k, at.slot0, n) : view_row_word(q, d, at.slot0, n);
    int64_t row;
    if (src_of >= SRC_T4) {
        const int t = src_of - SRC_T4;
        const int cnt = (int)m[10 + t];
        if (cnt == 0) {                                            // the ingest raised err for this clip: void views
            view_void(dst);
            if (io) *io = -1;
            return;
        }
        row = m[0] + lists[2 * m[9] + t * m[4] + draw_row(word, cnt)];
    } else {
        row = m[src_of] + draw_row(word, (int)m[4 + src_of]);
    }
    if (io) *io = row;
    if (REF) view_point_reference<S>(src + row * RC, q, at.k, at.slot0, n, dst);
    else view_point<S>(src + row * RC, q, rc, d, at.slot0, n, dst);
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
    if (!src || !table || !lists || !sel || !out || !err) return FACL_E_NULL;
    if (n_clips < 1 || B < 1 || B > (1 << 20) || !views_gp_ok(G, P)) return FACL_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) % 16) return FACL_E_ALIGN;
    const ViewGrid g = view_grid(P);
    const auto kernel = view_recipe_is_default(rc) ? k_build_views_resident<S, true> : k_build_views_resident<S, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B * G * g.chunks), dim3(g.threads), 0, (hipStream_t)stream, src, table, lists,
                       n_clips, sel, B, G, P, g.chunks, seed, epoch, out, idx_out, err, rc);
    return facl_launch_status();
}

// the recipe entries: the caller's HOST arrays are checked and turned into the recipe first (no launch on a refusal)
template <typename S>
static int launch_views_resident_recipe(const S* src, const int64_t* table, const int32_t* lists, int n_clips,
                                        const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                        int64_t* idx_out, int32_t* err, const int32_t* kinds, int n_kinds,
                                        const double* strengths, void* stream) {
    ViewRecipe rc;
    const int e = view_recipe_make(kinds, n_kinds, strengths, &rc);
    if (e != 0) return e;
    return launch_views_resident<S>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err, rc, stream);
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
    return launch_views_resident_recipe<float>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err, kinds,
                                               n_kinds, strengths, stream);
}

extern "C" int facl_build_views_resident_recipe_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                                    const int32_t* sel, int B, int G, int P, int64_t seed, int epoch,
                                                    float* out, int64_t* idx_out, int32_t* err, const int32_t* kinds,
                                                    int n_kinds, const double* strengths, void* stream) {
    return launch_views_resident_recipe<double>(src, table, lists, n_clips, sel, B, G, P, seed, epoch, out, idx_out, err,
                                                kinds, n_kinds, strengths, stream);
}
