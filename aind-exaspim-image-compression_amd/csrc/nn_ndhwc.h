// nn_ndhwc.h -- what the forward (nn_kernels.hip) and backward (nn_grad_kernels.hip) NDHWC kernels of the BM4DNet
// stage must agree on bit for bit: the per-axis source indices and weights of the x2 align-corners interpolation.
#pragma once
#include <hip/hip_runtime.h>

namespace exabm4d {

// out extent = 2 * in; source coordinate r * o with r = (in - 1) / (out - 1) in fp32, i0 = (int)(r o),
// i1 = i0 + (i0 < in - 1), weights (1 - lambda, lambda): PyTorch's upsample_trilinear3d with align_corners
struct UpAxis {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ UpAxis up_axis(int o, int in, float r) {
    const float src = r * (float)o;
    UpAxis a;
    a.i0 = (int)src;
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.w1 = src - (float)a.i0;
    a.w0 = 1.0f - a.w1;
    return a;
}
// r of an axis of input extent `in` (output 2 * in), as both launchers pass it
inline float up_ratio(int in) { return 2 * in > 1 ? (float)(in - 1) / (float)(2 * in - 1) : 0.0f; }

}  // namespace exabm4d
