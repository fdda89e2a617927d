// sampler_kernels.hip -- DESIGN.md 5.15: what the patch samplers of the reference's data_handling.py:446-702 score
// and rasterise, on batches of patches (B, nz, ny, nx) in HBM (gfx950).
//
//   count_kernel          per patch, the number of voxels that are set in a source or (iterate) have a face
//                         neighbour inside the patch that is: int(dilated mask .sum()) without the mask.  One
//                         workgroup per (patch, slab of z); a wave counts by ballot + popcount, the workgroup makes
//                         one integer add.  The rule and the border are dilate_kernel's (mask_kernels.hip).
//   raster_points_kernel  make_skeleton_mask's rasteriser for many boxes: grid-stride over the points, the launch's
//                         box origins in LDS, a byte store of 1 into every box that contains the point.
//   or_bytes_kernel       out |= in over 0 / 1 bytes.
//
// Everything here is integers and bytes: the results do not depend on the launch shape or on the batch.
#include "exabm4d_kernels.h"
#include "mask_src.h"

namespace exabm4d {

constexpr int CNT_T = 256;
constexpr int CNT_W = CNT_T / 64;
constexpr size_t CNT_SLAB = 16384;   // voxels a workgroup counts, rounded up to whole planes

template <class Src>
__global__ __launch_bounds__(CNT_T) void count_kernel(Src src, int nz, int ny, int nx, int slab_z, int slabs,
                                                      int iterate, uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[CNT_W];
    const size_t plane = (size_t)ny * nx, n = plane * nz;
    const int b = blockIdx.x / slabs, z0 = (blockIdx.x % slabs) * slab_z;
    const int z1 = z0 + slab_z < nz ? z0 + slab_z : nz;
    const size_t off = (size_t)b * n, end = plane * z1;
    const auto one = src.patch(b);
    uint32_t cnt = 0;   // the same in every lane of a wave
    for (size_t base = plane * z0; base < end; base += CNT_T) {   // uniform trip count: every lane ballots
        const size_t v = base + threadIdx.x;
        bool m = false;
        if (v < end) {
            const size_t i = off + v;
            m = one(i);
            if (iterate && !m) {
                // a patch has fewer than 2^32 voxels: 32-bit divisions
                const uint32_t row = (uint32_t)v / (uint32_t)nx;
                const int x = (int)((uint32_t)v - row * (uint32_t)nx), z = (int)(row / (uint32_t)ny);
                const int y = (int)(row - (uint32_t)z * (uint32_t)ny);
                m = (x > 0 && one(i - 1)) || (x + 1 < nx && one(i + 1)) ||
                    (y > 0 && one(i - nx)) || (y + 1 < ny && one(i + nx)) ||
                    (z > 0 && one(i - plane)) || (z + 1 < nz && one(i + plane));
            }
        }
        cnt += (uint32_t)__popcll(__ballot(m));
    }
    if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < CNT_W; w++) s += part[w];
        if (s) atomicAdd(&counts[b], s);
    }
}

// z planes per workgroup: about CNT_SLAB voxels, whole planes
static int slab_planes(int nz, int ny, int nx) {
    const size_t plane = (size_t)ny * nx;
    const size_t sz = (CNT_SLAB + plane - 1) / plane;
    return sz < (size_t)nz ? (int)sz : nz;
}

long long count_workgroups(int batch, int nz, int ny, int nx) {
    const int slab_z = slab_planes(nz, ny, nx);
    return (long long)batch * ((nz + slab_z - 1) / slab_z);
}

template <class Src>
static hipError_t count_from(Src src, int batch, int nz, int ny, int nx, int iterate, uint32_t* counts,
                             hipStream_t s) {
    const int slab_z = slab_planes(nz, ny, nx), slabs = (nz + slab_z - 1) / slab_z;
    // counts are zeroed here, on the stream; the caller has bounded count_workgroups() below 2^31
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)batch * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(count_kernel<Src>, dim3((unsigned)batch * (unsigned)slabs), dim3(CNT_T), 0, s, src, nz, ny,
                       nx, slab_z, slabs, iterate, counts);
    return hipGetLastError();
}

hipError_t launch_count_above(const void* raw, int dtype, const float* thr, int batch, int nz, int ny, int nx,
                              int iterate, uint32_t* counts, hipStream_t s) {
    const size_t n = (size_t)nz * ny * nx;
    if (dtype == 0)
        return count_from(AboveThr<uint16_t>{(const uint16_t*)raw, thr, n}, batch, nz, ny, nx, iterate, counts, s);
    return count_from(AboveThr<float>{(const float*)raw, thr, n}, batch, nz, ny, nx, iterate, counts, s);
}

hipError_t launch_count_mask(const uint8_t* mask, int batch, int nz, int ny, int nx, int iterate, uint32_t* counts,
                             hipStream_t s) {
    return count_from(MaskSrc{mask}, batch, nz, ny, nx, iterate, counts, s);
}

// ---- skeleton points into many boxes --------------------------------------------------------------------------
constexpr int RB_T = 256;

__global__ __launch_bounds__(RB_T) void raster_points_kernel(const int32_t* __restrict__ pts, size_t npts,
                                                             const int32_t* __restrict__ starts, int nbox, int nz,
                                                             int ny, int nx, RasterBounds bb,
                                                             uint8_t* __restrict__ out) {
    __shared__ int32_t origin[RASTER_BOXES * 3];
    for (int i = threadIdx.x; i < nbox * 3; i += RB_T) origin[i] = starts[i];
    __syncthreads();
    const size_t n = (size_t)nz * ny * nx;
    for (size_t i = (size_t)blockIdx.x * RB_T + threadIdx.x; i < npts; i += (size_t)gridDim.x * RB_T) {
        const long long z = pts[3 * i], y = pts[3 * i + 1], x = pts[3 * i + 2];
        if (z < bb.lo[0] || z >= bb.hi[0] || y < bb.lo[1] || y >= bb.hi[1] || x < bb.lo[2] || x >= bb.hi[2])
            continue;   // outside every box of this launch
        for (int b = 0; b < nbox; b++) {
            const long long dz = z - origin[3 * b], dy = y - origin[3 * b + 1], dx = x - origin[3 * b + 2];
            if (dz >= 0 && dz < nz && dy >= 0 && dy < ny && dx >= 0 && dx < nx)
                out[(size_t)b * n + ((size_t)dz * ny + (size_t)dy) * nx + (size_t)dx] = 1;   // equal stores may race
        }
    }
}

hipError_t launch_raster_points(const int32_t* pts, size_t npts, const int32_t* starts, int nbox, int nz, int ny,
                                int nx, const RasterBounds& bb, uint8_t* out, hipStream_t s) {
    size_t g = (npts + RB_T - 1) / RB_T;
    if (g > 1024) g = 1024;
    if (g == 0) return hipSuccess;
    hipLaunchKernelGGL(raster_points_kernel, dim3((unsigned)g), dim3(RB_T), 0, s, pts, npts, starts, nbox, nz, ny, nx,
                       bb, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(RB_T) void or_bytes_kernel(const uint8_t* __restrict__ in, size_t total,
                                                        uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * RB_T + threadIdx.x; i < total; i += (size_t)gridDim.x * RB_T)
        if (in[i]) out[i] = 1;
}

hipError_t launch_or_bytes(const uint8_t* in, size_t total, uint8_t* out, hipStream_t s) {
    size_t g = (total + RB_T - 1) / RB_T;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(or_bytes_kernel, dim3((unsigned)(g ? g : 1)), dim3(RB_T), 0, s, in, total, out);
    return hipGetLastError();
}

}  // namespace exabm4d
