// nn_ndhwc.h -- what the forward (nn_kernels.hip) and backward (nn_grad_kernels.hip) NDHWC kernels of the BM4DNet
// stage must agree on bit for bit: the per-axis source indices and weights of the x2 align-corners interpolation,
// and how four channels of a storage type are widened to fp32 and rounded back.
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

// Four consecutive channels in storage type T: Pack<T>::type is what one thread loads or stores, unpack widens
// it to fp32 exactly, pack rounds each element once, to nearest even (v_cvt_f16_f32 / v_cvt_pk_bf16_f32).
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
template <typename T> struct Pack;
template <> struct Pack<float> {
    using type = float4;
    static __device__ __forceinline__ float4 unpack(const float4 v) { return v; }
    static __device__ __forceinline__ float4 pack(const float4 v) { return v; }
};
template <typename V> struct HalfPack {
    using type = V;
    static __device__ __forceinline__ float4 unpack(const V v) {
        const float4_t f = __builtin_convertvector(v, float4_t);
        return make_float4(f.x, f.y, f.z, f.w);
    }
    static __device__ __forceinline__ V pack(const float4 v) {
        const float4_t f = {v.x, v.y, v.z, v.w};
        return __builtin_convertvector(f, V);
    }
};
template <> struct Pack<_Float16> : HalfPack<half4_t> {};
template <> struct Pack<__bf16> : HalfPack<bf16x4_t> {};

}  // namespace exabm4d
