// Row body of the L2-normalisation passes (F.normalize: x / max(||x||_2, 1e-12)) shared by the classifier head's gather + normalise
// (cls.hip: one workgroup per clip) and the contrastive loss's row pass (loss.hip: one wave per row).  A thread accumulates the
// float4s it strides over in fp64, components in the order x, y, z, w; the caller reduces the per-thread sums in its own fixed
// order (wave xor tree, then the waves in order) and rounds ONCE to fp32 through the helpers below.
#pragma once
#include "common.h"

__device__ __forceinline__ void nr_acc_sq(double& ss, const float4 v) {
    ss += (double)v.x * v.x; ss += (double)v.y * v.y; ss += (double)v.z * v.z; ss += (double)v.w * v.w;
}

__device__ __forceinline__ void nr_acc_dot(double& dot, const float4 d, const float4 o) {
    dot += (double)d.x * o.x; dot += (double)d.y * o.y; dot += (double)d.z * o.z; dot += (double)d.w * o.w;
}

// 1 / max(||x||, eps) in fp64 from the sum of squares (F.normalize's clamp)
__device__ __forceinline__ double nr_inv_norm(double ss) {
    const double nrm = sqrt(ss);
    return 1.0 / (nrm > 1e-12 ? nrm : 1e-12);
}

__device__ __forceinline__ float4 nr_scale_f32(float4 v, float inv) {
    v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    return v;
}

// fp64 scale, one rounding per element
__device__ __forceinline__ float4 nr_scale_f64(const float4 v, double sc) {
    float4 r;
    r.x = (float)((double)v.x * sc); r.y = (float)((double)v.y * sc);
    r.z = (float)((double)v.z * sc); r.w = (float)((double)v.w * sc);
    return r;
}

// gradient of o = x * inv through the normalisation: inv * (d - o <d, o>), one rounding per element
__device__ __forceinline__ float4 nr_project(double inv, const float4 d, const float4 o, double dot) {
    float4 r;
    r.x = (float)(inv * ((double)d.x - (double)o.x * dot));
    r.y = (float)(inv * ((double)d.y - (double)o.y * dot));
    r.z = (float)(inv * ((double)d.z - (double)o.z * dot));
    r.w = (float)(inv * ((double)d.w - (double)o.w * dot));
    return r;
}
