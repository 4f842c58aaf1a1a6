// View construction of a batch of clips (cn3D_data_set.py:285-350 get_data_train, :654-663, :708-713,
// :734-749, :767-778): gather-with-replacement, jitter, x-mirror, y-rotation, temporal-channel select, float64 ->
// float32 and the (B,G,N,D) -> view-major (G*B,N,D) re-layout of cn3d_train_motion_GL.py:225-228, in ONE launch.
// The reference draws every random number from NumPy's global generator; to stay reproducible against it the HOST
// draws them in the reference's order (facl_amd/views.py) and this kernel consumes them: row indices (already
// composed with the non-zero filter of the temporal views), the standard-normal jitter draws and cos/sin of the two
// rotation angles (evaluated by NumPy in float64).  The arithmetic is view_chain_reference of views_point.inc, the chain
// the philox kernels run at the default recipe on their own draws.  HBM-bound: 16 B written per point.
#include "common.h"

namespace {

constexpr int NV = 10, NP = 512, NJ = 7;   // views, points per view (NUM_POINT, :24), jitter draws per clip

#include "views_point.inc"

// block = one (clip, view); thread = one point
template <typename S>
__global__ __launch_bounds__(NP) void k_build_views(const S* __restrict__ src, int C, const int* __restrict__ idx,
                                                    const double* __restrict__ noise, const double* __restrict__ cs,
                                                    int B, float* __restrict__ out) {
    const int b = blockIdx.x / NV, v = blockIdx.x % NV, n = threadIdx.x;
    const long long row = idx[((size_t)b * NV + v) * NP + n];
    // jitter slots per clip: rev 0,1 | ke1 2 | ke2 3,4 | ro1 5 | ro2 6
    const double* nz = noise + ((size_t)b * NJ * NP + n) * 3;
    view_chain_reference<S>(
        src + row * C, v, [&](int slot, int d) -> double { return jit(nz[(size_t)slot * NP * 3 + d], 0.01, 0.05); },
        [&](int k) -> CosSin { return {cs[((size_t)b * 2 + k) * 2], cs[((size_t)b * 2 + k) * 2 + 1]}; },
        out + (((size_t)v * B + b) * NP + n) * 4);               // view-major row g*B + b
}

}  // namespace

template <typename S>
static int launch_views(const S* src, int64_t rows, int C, const int* idx, const double* noise, const double* cs, int B,
                        float* out, void* stream) {
    if (!src || !idx || !noise || !cs || !out) return FACL_E_NULL;
    if (B < 1 || rows < 1 || C < 8 || B > (1 << 20)) return FACL_E_SHAPE;
    hipLaunchKernelGGL((k_build_views<S>), dim3(B * NV), dim3(NP), 0, (hipStream_t)stream, src, C, idx, noise, cs, B, out);
    return facl_launch_status();
}

extern "C" int facl_build_views_f32(const float* src, int64_t rows, int C, const int32_t* idx, const double* noise,
                                    const double* cossin, int B, float* out, void* stream) {
    return launch_views<float>(src, rows, C, idx, noise, cossin, B, out, stream);
}

extern "C" int facl_build_views_f64(const double* src, int64_t rows, int C, const int32_t* idx, const double* noise,
                                    const double* cossin, int B, float* out, void* stream) {
    return launch_views<double>(src, rows, C, idx, noise, cossin, B, out, stream);
}
