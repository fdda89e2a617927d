// foreground_kernels.hip -- the foreground mask of a box inside a window: threshold, bit
// packing by ballot and every dilation iteration in ONE launch, on packed 64-bit words in LDS.
//
//   out[b] = value  if some voxel p of the VOLUME has vol[p] >= cut and |p - b|_1 <= radius,  else 0
//
// for every voxel b of the box -- `radius` iterations of the 6-neighbour cross with border 0 are one dilation by the
// L1 ball, cut at the volume's faces, so a box depends only on the voxels within `radius` of it per axis.
//
// A workgroup of FG_T = 512 threads (8 waves) owns a REGION of FG_N x FG_N rows (z, y) of 512 voxels in x: 64 lanes
// times 8 voxels, one 16-byte load per lane and row.  The eight comparisons of a lane become eight ballots, so a row
// is kept as eight 64-bit PLANES: bit l of plane e is voxel 8 l + e of the row.  A region is FG_N^2 x 8 words = 64 KiB
// of LDS (two workgroups per CU).  In that layout one iteration of the cross is, per word,
//
//   w'[e] = w[e] | w[e - 1] | w[e + 1] | w[e](y - 1) | w[e](y + 1) | w[e](z - 1) | w[e](z + 1),
//   with w[-1] = w[7] << 1 and w[8] = w[0] >> 1   (the voxel before 8 l + 0 is 8 (l - 1) + 7):
//
// two shifts per row instead of two per word, and no carries between words, because a region is one row of planes
// wide.  What lies outside the region counts as 0, so after i iterations the outermost i rows and voxels of the region
// are wrong; the region's outputs are its rows radius .. FG_N - radius - 1 and 488 voxels that begin 8 .. 15 voxels
// into it and end at least 9 before its end (radius <= 8).  The final pass reads a row's planes back (one broadcast
// read per plane), lets lane j assemble the eight voxels of its output vector -- which begins at any voxel of the
// region, so loads and stores are 16-byte aligned each in its own phase -- and stores 16 bytes (8 for the byte form).
//
// A voxel is a seed only where it lies inside the volume AND inside the part of the window the box needs: a reader's
// padding past the volume's faces (65535) is never a seed, whatever `cut` is.
#include <algorithm>

#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int FG_T = 512;
constexpr int FG_WAVES = FG_T / 64;
constexpr int FG_N = 32;                    // rows of a region per axis (z, y)
constexpr int FG_ROWS = FG_N * FG_N;
constexpr int FG_WORDS = FG_ROWS * 8;       // 64-bit words of a region
constexpr int FG_PER_THREAD = FG_WORDS / FG_T;
constexpr size_t FG_LDS_BYTES = (size_t)FG_WORDS * 8 + 2 * FG_WAVES * 8;

static_assert(FG_MAX_RADIUS == 8, "the x halo of a region is one lane (8 voxels) on either side");
static_assert(FG_N == 32 && FG_N - 2 * FG_MAX_RADIUS >= 1, "row indices are split by shifts");

// eight voxels of a row as four dwords; `aligned`: a 16-byte aligned address
__device__ __forceinline__ void fg_load8(const uint16_t* __restrict__ p, bool aligned, uint32_t (&d)[4]) {
    if (aligned) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) d[e] = (uint32_t)p[2 * e] | ((uint32_t)p[2 * e + 1] << 16);
    }
}

__global__ __launch_bounds__(FG_T) void foreground_box_kernel(const uint16_t* __restrict__ win, BoxGeom g, FgPlan p,
                                                              uint32_t cut, int radius, uint32_t value,
                                                              uint16_t* __restrict__ out16,
                                                              uint8_t* __restrict__ out8,
                                                              unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned long long fg_lds[];
    unsigned long long* W = fg_lds;                      // [FG_ROWS][8]
    unsigned long long* red = fg_lds + FG_WORDS;         // [2][FG_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int span = FG_N - 2 * radius;                  // output rows of a region per axis
    const int tz0 = g.b0[0] - radius + (int)blockIdx.z * span;
    const int ty0 = g.b0[1] - radius + (int)blockIdx.y * span;
    const int tx0 = p.xs + (int)blockIdx.x * FG_STRIDE_X;
    const int bz1 = g.b0[0] + g.bd[0], by1 = g.b0[1] + g.bd[1], bx1 = g.b0[2] + g.bd[2];
    const int out_x0 = tx0 + 8 + p.shift;                // the region's first output vector begins here
    const int own_x0 = max(g.b0[2], out_x0), own_x1 = min(bx1, out_x0 + FG_STRIDE_X);

    // ---- pass 1: load, compare, pack -------------------------------------------------------------------------
    const int xg = tx0 + 8 * lane;                       // this lane's eight voxels of every row
    uint32_t readable = 0, owned = 0;                    // per element: may be a seed / is counted by this region
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int x = xg + e;
        if (x >= p.r0[2] && x < p.r1[2]) readable |= 1u << e;
        if (x >= own_x0 && x < own_x1) owned |= 1u << e;
    }
    const bool whole = readable == 0xFFu;
    uint32_t nseed = 0;
    for (int r0 = wave; r0 < FG_ROWS; r0 += 4 * FG_WAVES) {
        uint32_t d[4][4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u * FG_WAVES;
            const int z = tz0 + (r >> 5), y = ty0 + (r & 31);
            ok[u] = z >= p.r0[0] && z < p.r1[0] && y >= p.r0[1] && y < p.r1[1];
            d[u][0] = d[u][1] = d[u][2] = d[u][3] = 0u;
            if (!ok[u] || !readable) continue;
            const uint16_t* row = win + ((size_t)(z - g.w0[0]) * g.wd[1] + (size_t)(y - g.w0[1])) * (size_t)g.wd[2];
            if (whole) {
                fg_load8(row + (xg - g.w0[2]), p.vec_in != 0, d[u]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (readable >> e & 1u) d[u][e >> 1] |= (uint32_t)row[xg + e - g.w0[2]] << ((e & 1) * 16);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u * FG_WAVES;
            uint32_t seeds = 0;
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (((d[u][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu) >= cut) seeds |= 1u << e;
            seeds = ok[u] ? seeds & readable : 0u;
            unsigned long long mine = 0ull;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const unsigned long long b = __ballot((seeds >> e) & 1u);
                if (lane == e) mine = b;
            }
            if (lane < 8) W[r * 8 + lane] = mine;
            const int zr = r >> 5, yr = r & 31, z = tz0 + zr, y = ty0 + yr;
            if (zr >= radius && zr < FG_N - radius && yr >= radius && yr < FG_N - radius && z >= g.b0[0] && z < bz1 &&
                y >= g.b0[1] && y < by1)
                nseed += __popc(seeds & owned);
        }
    }
    __syncthreads();

    // ---- the iterations: every thread FG_PER_THREAD words, new values held in registers between the barriers ----
    for (int it = 0; it < radius; it++) {
        unsigned long long nw[FG_PER_THREAD];
#pragma unroll
        for (int k = 0; k < FG_PER_THREAD; k++) {
            const int i = tid + k * FG_T;
            const int e = i & 7, r = i >> 3, zr = r >> 5, yr = r & 31;
            const unsigned long long* row = W + (r << 3);
            unsigned long long w = row[e];
            const unsigned long long lo = row[(e + 7) & 7], hi = row[(e + 1) & 7];
            w |= e == 0 ? lo << 1 : lo;
            w |= e == 7 ? hi >> 1 : hi;
            if (yr > 0) w |= W[i - 8];
            if (yr < FG_N - 1) w |= W[i + 8];
            if (zr > 0) w |= W[i - 8 * FG_N];
            if (zr < FG_N - 1) w |= W[i + 8 * FG_N];
            nw[k] = w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FG_PER_THREAD; k++) W[tid + k * FG_T] = nw[k];
        __syncthreads();
    }

    // ---- the final pass: lane j assembles the output vector that begins at voxel 8 (j + 1) + shift of the region --
    uint32_t nfg = 0;
    const int xv = out_x0 + 8 * lane;
    uint32_t inbox = 0;
    if (lane < FG_LANES_OUT) {
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (xv + e >= g.b0[2] && xv + e < bx1) inbox |= 1u << e;
    }
    for (int q = wave; q < span * span; q += FG_WAVES) {
        const int zr = radius + q / span, yr = radius + q % span;
        const int z = tz0 + zr, y = ty0 + yr;
        if (z >= bz1 || y >= by1 || !inbox) continue;    // (z >= b0 and y >= b0 hold for every output row)
        const unsigned long long* row = W + ((zr * FG_N + yr) << 3);
        uint32_t m = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int idx = p.shift + e;
            m |= (uint32_t)((row[idx & 7] >> ((lane + 1 + (idx >> 3)) & 63)) & 1ull) << e;
        }
        m &= inbox;
        nfg += __popc(m);
        const long long o = ((long long)(z - g.b0[0]) * g.bd[1] + (y - g.b0[1])) * (long long)g.bd[2] + (xv - g.b0[2]);
        if (out16) {
            if (p.vec_u16 && inbox == 0xFFu) {
                uint4 v;
                v.x = ((m & 1u) ? value : 0u) | ((m & 2u) ? value << 16 : 0u);
                v.y = ((m & 4u) ? value : 0u) | ((m & 8u) ? value << 16 : 0u);
                v.z = ((m & 16u) ? value : 0u) | ((m & 32u) ? value << 16 : 0u);
                v.w = ((m & 64u) ? value : 0u) | ((m & 128u) ? value << 16 : 0u);
                *reinterpret_cast<uint4*>(out16 + o) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (inbox >> e & 1u) out16[o + e] = (uint16_t)((m >> e & 1u) ? value : 0u);
            }
        }
        if (out8) {
            if (p.vec_u8 && inbox == 0xFFu) {
                uint2 v;
                v.x = (m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21;
                v.y = (m >> 4 & 1u) | (m >> 4 & 2u) << 7 | (m >> 4 & 4u) << 14 | (m >> 4 & 8u) << 21;
                *reinterpret_cast<uint2*>(out8 + o) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (inbox >> e & 1u) out8[o + e] = (uint8_t)(m >> e & 1u);
            }
        }
    }

    // ---- the counts: once per workgroup ----------------------------------------------------------------------
    if (!counts) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        nseed += (uint32_t)__shfl_xor((int)nseed, off);
        nfg += (uint32_t)__shfl_xor((int)nfg, off);
    }
    if (lane == 0) {
        red[wave] = nseed;
        red[FG_WAVES + wave] = nfg;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned long long t = 0ull;
        for (int w = 0; w < FG_WAVES; w++) t += red[tid * FG_WAVES + w];
        if (t) atomicAdd(&counts[tid], t);
    }
}

hipError_t foreground_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&foreground_box_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)FG_LDS_BYTES);
}

bool foreground_box_plan(const uint16_t* win, const BoxGeom& g, int radius, const uint16_t* out16, const uint8_t* out8,
                         FgPlan& p) {
    for (int a = 0; a < 3; a++) {
        p.r0[a] = std::max(std::max(g.w0[a], 0), g.b0[a] - radius);
        p.r1[a] = std::min(std::min(g.w0[a] + g.wd[a], g.n[a]), g.b0[a] + g.bd[a] + radius);
    }
    // output vectors: eight voxels from ox + 8 m, 16-byte aligned in out16 (8-byte in out8) where the box's pitch
    // keeps every row at one phase
    const bool pitch8 = g.bd[2] % 8 == 0;
    int ph = 0;
    p.vec_u16 = p.vec_u8 = 0;
    if (pitch8 && out16) {
        ph = (int)(((uintptr_t)out16 >> 1) & 7u);
        p.vec_u16 = 1;
        p.vec_u8 = out8 && (int)((uintptr_t)out8 & 7u) == ph;
    } else if (pitch8 && out8) {
        ph = (int)((uintptr_t)out8 & 7u);
        p.vec_u8 = 1;
    }
    const int ox = g.b0[2] - ph;
    // 16-byte loads: a pitch of whole vectors puts the aligned voxels of every row at x = first (mod 8)
    p.vec_in = g.wd[2] % 8 == 0;
    p.xs = ox - 8;
    if (p.vec_in) {
        const int first = (g.w0[2] - (int)(((uintptr_t)win >> 1) & 7u)) & 7;
        p.xs -= (p.xs - first) & 7;
    }
    p.shift = ox - 8 - p.xs;                             // 0 .. 7
    const int span = FG_N - 2 * radius;
    const long long slots = ((long long)g.b0[2] + g.bd[2] - ox + 7) / 8;
    const long long tx = (slots + FG_LANES_OUT - 1) / FG_LANES_OUT;
    const long long ty = ((long long)g.bd[1] + span - 1) / span, tz = ((long long)g.bd[0] + span - 1) / span;
    if (tx > 0x7FFFFFFFll || ty > 65535 || tz > 65535) return false;
    p.tiles[0] = (unsigned)tx;
    p.tiles[1] = (unsigned)ty;
    p.tiles[2] = (unsigned)tz;
    return true;
}

hipError_t launch_foreground_box_u16(const uint16_t* win, const BoxGeom& g, const FgPlan& p, uint32_t cut, int radius,
                                     uint32_t value, uint16_t* out16, uint8_t* out8, unsigned long long* counts,
                                     hipStream_t s) {
    hipLaunchKernelGGL(foreground_box_kernel, dim3(p.tiles[0], p.tiles[1], p.tiles[2]), dim3(FG_T), FG_LDS_BYTES, s, win,
                       g, p, cut, radius, value, out16, out8, counts);
    return hipGetLastError();
}

}  // namespace exabm4d
