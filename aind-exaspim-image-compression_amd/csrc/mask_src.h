// mask_src.h -- the voxel sources of the mask kernels (mask_kernels.hip, sampler_kernels.hip): a source says
// whether voxel i of a batch of patches (n voxels each, contiguous) is set.
#pragma once
#include "exabm4d_common.h"

namespace exabm4d {

// patch(b): the same source for a caller that knows voxel i lies in patch b (no 64-bit i / n per voxel)
template <class T>
struct AboveOne {
    const T* p;
    float t;
    __device__ bool operator()(size_t i) const { return (float)p[i] > t; }
};
template <class T>
struct AboveThr {
    const T* p;
    const float* thr;
    size_t n;
    __device__ bool operator()(size_t i) const { return (float)p[i] > thr[i / n]; }
    __device__ AboveOne<T> patch(size_t b) const { return AboveOne<T>{p, thr[b]}; }
};
struct MaskSrc {
    const uint8_t* p;
    __device__ bool operator()(size_t i) const { return p[i] != 0; }
    __device__ MaskSrc patch(size_t) const { return *this; }
};
// labels > 0: make_segmentation_mask's source (ids <= 0 of the signed types are background)
template <class T>
struct LabelSrc {
    const T* p;
    __device__ bool operator()(size_t i) const { return p[i] > (T)0; }
};

}  // namespace exabm4d
