// bounded_pairs.h -- what the two error-bounded codecs share (bounded_kernels.hip: a step per chunk, DESIGN.md 3.10b;
// block_bounded_kernels.hip: a step per 8^3 block): the blocks of a chunk, the load of a block pair,
// the quantiser's rounding and the launch geometry.  A wave owns a pair of x-adjacent blocks (dct_pairs.h).
#pragma once
#include "dct_pairs.h"
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int BQ_WAVES = 4;
constexpr int BQ_PAIRS = 16;                 // block pairs per wave and workgroup (a chunk takes several workgroups)
constexpr float BQ_IDX_MAX = 1073741824.0f;  // indices are clamped to +-2^30

__device__ __forceinline__ int bq_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the blocks of chunk c: first block in the volume's block grid, and ceil(E / 8) blocks per axis inside the volume
struct BqChunkBlocks {
    int bz0, by0, bx0;
    int lbz, lby, lbx;
};
__device__ __forceinline__ BqChunkBlocks bq_chunk_blocks(const BoundedGeom& g, int c) {
    const int kx = c % g.gx, ky = (c / g.gx) % g.gy, kz = c / (g.gx * g.gy);
    BqChunkBlocks b;
    b.bz0 = kz * g.cbz;
    b.by0 = ky * g.cby;
    b.bx0 = kx * g.cbx;
    b.lbz = min(g.cbz, (g.nz - kz * g.cz + 7) / 8);
    b.lby = min(g.cby, (g.ny - ky * g.cy + 7) / 8);
    b.lbx = min(g.cbx, (g.nx - kx * g.cx + 7) / 8);
    return b;
}

// layout L1 (lane = (z, x), registers = y) of two x-adjacent blocks, edge voxels replicated: dctq_forward_kernel's load
__device__ __forceinline__ void bq_load_pair(const uint16_t* __restrict__ vol, const BoundedGeom& g, int bz, int by,
                                             int bxa, int bxb, int hi, int lo, f2 (&v)[8]) {
    const size_t zrow = (size_t)bq_clamp(8 * bz + hi, 0, g.nz - 1) * g.ny;
    const int xa = bq_clamp(8 * bxa + lo, 0, g.nx - 1), xb = bq_clamp(8 * bxb + lo, 0, g.nx - 1);
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const size_t row = (zrow + bq_clamp(8 * by + y, 0, g.ny - 1)) * g.nx;
        v[y] = mk2((float)vol[row + xa], (float)vol[row + xb]);
    }
}

__device__ __forceinline__ int32_t bq_quantise(float c, float q) {
    return (int32_t)fminf(fmaxf(rintf(c / q), -BQ_IDX_MAX), BQ_IDX_MAX);
}

__device__ __forceinline__ float bq_to_voxel(float v) { return rintf(fminf(fmaxf(v, 0.0f), 65535.0f)); }

// workgroups per chunk so that a wave takes about BQ_PAIRS block pairs of a full chunk
inline int bq_slices(const BoundedGeom& g) {
    const long long pairs = (long long)g.cbz * g.cby * ((g.cbx + 1) / 2);
    const long long s = (pairs + BQ_WAVES * BQ_PAIRS - 1) / (BQ_WAVES * BQ_PAIRS);
    return (int)(s < 1 ? 1 : s);
}

inline bool bq_grid(const BoundedGeom& g, unsigned& grid, int& slices) {
    slices = bq_slices(g);
    const long long n = (long long)g.nchunks * slices;
    if (n > 0x7FFFFFFFll) return false;
    grid = (unsigned)n;
    return true;
}

inline bool bq_table(const float* dct64, Dct7& q7) {
    DctTable T;
    for (int i = 0; i < 64; i++) T.d[i] = dct64[i];
    return make_dct7(T, q7);
}

}  // namespace exabm4d
