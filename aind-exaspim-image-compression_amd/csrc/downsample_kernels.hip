// downsample_kernels.hip -- one pyramid level of a box inside a window: every voxel of a box
// of the LEVEL reduces the window fz x fy x fx (each 1 or 2) of the SOURCE volume that begins at its index times the
// factors, cut at the volume's faces, by its mode (ties: the smallest value), its mean (half to even) or its maximum.
//
// A stream: 2 bytes in per source voxel, 2 bytes out per level voxel, no LDS, no atomics.  A lane owns a PIECE: eight
// source voxels of a row (16 bytes), hence 8 / fx outputs; it reads that piece from the fz fy source rows of its output
// row and stores 8 bytes (16 with fx = 1).  Pieces begin at the level x `ox + p (8 / fx)`, where ox = box x - oshift and
// the host picks oshift (0 .. 8 / fx - 1) so that the pieces of every row are 16-byte aligned in the window.
//
// A window shorter than 8 voxels -- a factor of 1, or an axis cut by a face under edge = "partial" -- is filled up by
// REPEATING along that axis the voxel that is present.  That doubles the frequency of every value present alike (and the
// sum together with the count), so the mode, its tie rule, the mean and the maximum of the voxels present are unchanged:
// nothing but voxels of the volume ever enters the network, whatever a reader's padding past the faces holds.  The mode
// of the 8 (4 with fx = 1: one voxel per row, the x axis needs no repeats) values is a fixed compare-exchange network in
// registers and a scan of the runs of the sorted values; the first longest run wins, which is the smallest value.
//
// 16-byte loads are taken where (downsample_box_plan) the window's pitch is a multiple of 8 voxels and, with fx = 2, the
// box's first source voxel lies at an even element of the window's allocation -- then some oshift aligns every piece --,
// for the pieces that lie whole inside a window row.  8- / 16-byte stores are taken where the box's pitch is a multiple
// of 8 / fx, the output pointer's phase equals the pieces' (always, when the loads could not choose oshift), for the
// pieces that lie whole inside the box.  Everything else goes element by element.
#include <algorithm>

#include "ds_sort.h"
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int DS_T = 256;

// the reduction of N = 4 or 8 values (repeats included)
template <int METHOD, int N>
__device__ __forceinline__ uint32_t ds_reduce(uint32_t (&v)[N]) {
    if constexpr (METHOD == DS_MAX) {
        uint32_t m = v[0];
#pragma unroll
        for (int i = 1; i < N; i++) m = max(m, v[i]);
        return m;
    } else if constexpr (METHOD == DS_MEAN) {
        constexpr int SH = N == 8 ? 3 : 2;
        uint32_t s = 0;
#pragma unroll
        for (int i = 0; i < N; i++) s += v[i];
        return (s + ((1u << (SH - 1)) - 1u) + ((s >> SH) & 1u)) >> SH;        // sum / N, half to even
    } else {
        ds_sort(v);
        uint32_t best = v[0], best_len = 1, run = 1;
#pragma unroll
        for (int i = 1; i < N; i++) {
            run = v[i] == v[i - 1] ? run + 1 : 1;
            if (run > best_len) {                    // (strictly: of runs of one length the first, the smallest value)
                best_len = run;
                best = v[i];
            }
        }
        return best;
    }
}

template <int FX, int METHOD>
__global__ __launch_bounds__(DS_T) void downsample_box_kernel(const uint16_t* __restrict__ win, BoxGeom g, DsPlan p,
                                                              uint16_t* __restrict__ out) {
    constexpr int OUTS = 8 / FX;
    const int bx1 = g.b0[2] + g.bd[2];
    // source x that may be read: the box's, cut at the volume (the window holds them: checked on the host)
    const int sx0 = g.b0[2] * FX, sx1 = min(g.n[2], bx1 * FX);
    for (int z = g.b0[0] + (int)blockIdx.z; z < g.b0[0] + g.bd[0]; z += (int)gridDim.z) {
        for (int y = g.b0[1] + (int)(blockIdx.y * blockDim.y + threadIdx.y); y < g.b0[1] + g.bd[1];
             y += (int)(gridDim.y * blockDim.y)) {
            // the source rows; a row past the volume, or of a factor of 1, repeats the one before it
            const uint16_t* rows[2][2];
#pragma unroll
            for (int dz = 0; dz < 2; dz++) {
#pragma unroll
                for (int dy = 0; dy < 2; dy++) {
                    const int zs = min(z * p.f[0] + (dz & (p.f[0] - 1)), g.n[0] - 1);
                    const int ys = min(y * p.f[1] + (dy & (p.f[1] - 1)), g.n[1] - 1);
                    rows[dz][dy] = win + ((size_t)(zs - g.w0[0]) * g.wd[1] + (size_t)(ys - g.w0[1])) * (size_t)g.wd[2];
                }
            }
            uint16_t* orow = out + ((size_t)(z - g.b0[0]) * g.bd[1] + (size_t)(y - g.b0[1])) * (size_t)g.bd[2];
            for (int pc = (int)(blockIdx.x * blockDim.x + threadIdx.x); pc < p.pieces; pc += (int)(gridDim.x * blockDim.x)) {
                const int xo = p.ox + pc * OUTS;                 // the piece's first output x (level)
                const int xs = xo * FX;                          // and its first source x
                uint32_t ok = 0;                                 // per element: a voxel of the box's source
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (xs + e >= sx0 && xs + e < sx1) ok |= 1u << e;
                const bool vec = p.vec_in && xs >= g.w0[2] && xs + 8 <= g.w0[2] + g.wd[2];
                uint32_t d[2][2][4];
#pragma unroll
                for (int dz = 0; dz < 2; dz++) {
#pragma unroll
                    for (int dy = 0; dy < 2; dy++) {
                        // a repeated row is copied in registers, not read again: fz fy rows are read per piece
                        const bool same_z = dz && rows[dz][dy] == rows[0][dy];
                        const bool same_y = dy && rows[dz][dy] == rows[dz][0];
                        if (same_z || same_y) {
#pragma unroll
                            for (int q = 0; q < 4; q++) d[dz][dy][q] = same_z ? d[0][dy][q] : d[dz][0][q];
                            continue;
                        }
                        const uint16_t* src = rows[dz][dy] + (xs - g.w0[2]);
                        if (vec) {
                            const uint4 v = *reinterpret_cast<const uint4*>(src);
                            d[dz][dy][0] = v.x; d[dz][dy][1] = v.y; d[dz][dy][2] = v.z; d[dz][dy][3] = v.w;
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; q++) d[dz][dy][q] = 0u;
#pragma unroll
                            for (int e = 0; e < 8; e++)
                                if (ok >> e & 1u) d[dz][dy][e >> 1] |= (uint32_t)src[e] << ((e & 1) * 16);
                        }
                    }
                }
                uint32_t r[OUTS];
#pragma unroll
                for (int j = 0; j < OUTS; j++) {
                    if constexpr (FX == 2) {
                        uint32_t v[8];
                        const bool second = ok >> (2 * j + 1) & 1u;      // else x is cut: repeat the first voxel
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t w = d[k >> 1][k & 1][j];
                            v[2 * k] = w & 0xFFFFu;
                            v[2 * k + 1] = second ? w >> 16 : w & 0xFFFFu;
                        }
                        r[j] = ds_reduce<METHOD, 8>(v);
                    } else {
                        uint32_t v[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) v[k] = (d[k >> 1][k & 1][j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
                        r[j] = ds_reduce<METHOD, 4>(v);
                    }
                }
                uint16_t* dst = orow + (xo - g.b0[2]);
                if (p.vec_out && xo >= g.b0[2] && xo + OUTS <= bx1) {
                    if constexpr (FX == 2) {
                        uint2 v;
                        v.x = r[0] | r[1] << 16;
                        v.y = r[2] | r[3] << 16;
                        *reinterpret_cast<uint2*>(dst) = v;
                    } else {
                        uint4 v;
                        v.x = r[0] | r[1] << 16;
                        v.y = r[2] | r[3] << 16;
                        v.z = r[4] | r[5] << 16;
                        v.w = r[6] | r[7] << 16;
                        *reinterpret_cast<uint4*>(dst) = v;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < OUTS; j++)
                        if (xo + j >= g.b0[2] && xo + j < bx1) dst[j] = (uint16_t)r[j];
                }
            }
        }
    }
}

void downsample_box_plan(const uint16_t* win, const BoxGeom& g, const int* factors, const uint16_t* out, DsPlan& p) {
    for (int a = 0; a < 3; a++) p.f[a] = factors[a];
    const int fx = factors[2], outs = 8 / fx;
    // the element of the window's allocation (mod 8) at which the box's first source voxel of every row lies
    const int phase = (int)((((uintptr_t)win >> 1) + (uintptr_t)(g.b0[2] * fx - g.w0[2])) & 7u);
    const bool pitch_out = g.bd[2] % outs == 0;
    const int out_phase = (int)(((uintptr_t)out >> 1) & (uintptr_t)(outs - 1));
    int oshift;
    p.vec_in = g.wd[2] % 8 == 0 && phase % fx == 0;
    if (p.vec_in) {
        oshift = phase / fx;                          // the pieces begin `phase` source voxels before the box
        p.vec_out = pitch_out && out_phase == oshift;
    } else {
        oshift = pitch_out ? out_phase : 0;
        p.vec_out = pitch_out;
    }
    p.ox = g.b0[2] - oshift;
    p.pieces = (g.bd[2] + oshift + outs - 1) / outs;
    // a wave covers 64 / bx rows where a row has fewer than 64 pieces
    int bx = 1;
    while (bx < 64 && bx < p.pieces) bx *= 2;
    p.block[0] = (unsigned)bx;
    p.block[1] = (unsigned)(DS_T / bx);
    p.grid[0] = (unsigned)((p.pieces + bx - 1) / bx);
    p.grid[1] = (unsigned)std::min<long long>(((long long)g.bd[1] + p.block[1] - 1) / p.block[1], 65535);
    p.grid[2] = (unsigned)std::min(g.bd[0], 65535);
}

hipError_t launch_downsample_box_u16(const uint16_t* win, const BoxGeom& g, const DsPlan& p, int method, uint16_t* out,
                                     hipStream_t s) {
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block[0], p.block[1]);
#define DS_LAUNCH(FX, M) hipLaunchKernelGGL((downsample_box_kernel<FX, M>), grid, block, 0, s, win, g, p, out)
    if (p.f[2] == 2) {
        if (method == DS_MODE) DS_LAUNCH(2, DS_MODE);
        else if (method == DS_MEAN) DS_LAUNCH(2, DS_MEAN);
        else DS_LAUNCH(2, DS_MAX);
    } else {
        if (method == DS_MODE) DS_LAUNCH(1, DS_MODE);
        else if (method == DS_MEAN) DS_LAUNCH(1, DS_MEAN);
        else DS_LAUNCH(1, DS_MAX);
    }
#undef DS_LAUNCH
    return hipGetLastError();
}

}  // namespace exabm4d
