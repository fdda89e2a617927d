// noise_cell.h -- one 2x2x2 cell of the noise table, shared by the kernels that count cells:
// noise_kernels.hip (a dense volume, one shift) and measure_kernels.hip (a box inside a window, every shift).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace exabm4d {

// the quarter-octave level of a cell sum s <= 8 * 65535
__device__ __forceinline__ int noise_level(uint32_t s) {
    const uint32_t t = (s >> 3) + 16u;
    const int e = 31 - __clz(t);                                   // 4 .. 16
    return 4 * (e - 4) + (int)((t >> (e - 2)) & 3u);               // 0 .. 48
}

// One cell of uint16 voxels: a, b, c, d are the dwords (x, x + 1) of the rows (z, y), (z, y + 1), (z + 1, y),
// (z + 1, y + 1).  s = the sum of the eight voxels, m = |sum of (-1)^(dz+dy+dx) v| <= 4 * 65535.
__device__ __forceinline__ void cell_u16_sm(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t& s, uint32_t& m) {
    const int a0 = a & 0xFFFFu, a1 = a >> 16, b0 = b & 0xFFFFu, b1 = b >> 16;
    const int c0 = c & 0xFFFFu, c1 = c >> 16, d0 = d & 0xFFFFu, d1 = d >> 16;
    s = (uint32_t)(a0 + a1 + b0 + b1 + c0 + c1 + d0 + d1);
    const int det = (a0 - a1) - (b0 - b1) - (c0 - c1) + (d0 - d1);
    m = (uint32_t)abs(det);
}

}  // namespace exabm4d
