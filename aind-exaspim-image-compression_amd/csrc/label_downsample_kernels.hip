// label_downsample_kernels.hip -- one pyramid level of a box of LABELS inside a window: the
// geometry and the shape of downsample_kernels.hip for uint32 / uint64 ids, which compare as unsigned integers.  Every
// voxel of a box of the LEVEL reduces the window fz x fy x fx (each 1 or 2) of the SOURCE volume that begins at its index
// times the factors, cut at the volume's faces, by its mode (ties: the smallest value); with ZEROS = LABEL_ZEROS_IGNORE
// by the mode of its non-zero values, 0 only where every voxel present is 0.
//
// A stream: no LDS, no atomics.  A lane owns a PIECE: 16 bytes of a source row, P = 4 (uint32) or 2 (uint64) voxels,
// hence P / fx outputs; it reads that piece from the fz fy source rows of its output row and stores 16 / fx bytes.
// Pieces begin at the level x `ox + p (P / fx)`, where ox = box x - oshift and the host picks oshift (0 .. P / fx - 1)
// so that the pieces of every row are 16-byte aligned in the window.
//
// A window shorter than 8 voxels -- a factor of 1, or an axis cut by a face under edge = "partial" -- is filled up by
// REPEATING along that axis the voxel that is present: that doubles the frequency of every value present alike, zeros
// included, so both reductions and their tie rule are unchanged, and nothing but voxels of the volume ever enters the
// network, whatever a reader's padding past the faces holds.  The mode of the 8 (4 with fx = 1) values: ds_sort's fixed
// network on whole keys, then a scan of the runs; the first longest run wins, which is the smallest value.  Zeros sort
// first, and under LABEL_ZEROS_IGNORE a run of zeros has length 0: no second pass.
//
// 16-byte loads are taken where (label_downsample_box_plan) the window's pitch is a multiple of P voxels and the box's
// first source voxel lies at a multiple of fx in the window's allocation (in elements, modulo P) -- then some oshift
// aligns every piece --, for the pieces that lie whole inside a window row.  Stores of 16 / fx bytes are taken where the
// box's pitch is a multiple of P / fx, the output pointer's phase equals the pieces', for the pieces that lie whole
// inside the box.  Everything else goes element by element.
#include <algorithm>

#include "ds_sort.h"
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int LBD_T = 256;          // threads of a workgroup
constexpr int LBD_PIECE = 16;       // bytes of a source row a lane takes

// the mode of N = 4 or 8 values (repeats included)
template <int ZEROS, typename T, int N>
__device__ __forceinline__ T label_mode(T (&v)[N]) {
    ds_sort(v);
    constexpr bool IGNORE = ZEROS == LABEL_ZEROS_IGNORE;
    T best = v[0];
    uint32_t best_len = IGNORE && v[0] == 0 ? 0u : 1u, run = best_len;
#pragma unroll
    for (int i = 1; i < N; i++) {
        run = v[i] == v[i - 1] ? run + 1 : 1;
        if (IGNORE && v[i] == 0) run = 0;            // (zeros sort first: a run of them never counts)
        if (run > best_len) {                        // (strictly: of runs of one length the first, the smallest value)
            best_len = run;
            best = v[i];
        }
    }
    return best;
}

// 32-bit word k of the outputs r as they lie in memory
template <typename T, int OUTS>
__device__ __forceinline__ uint32_t label_word(const T (&r)[OUTS], int k) {
    if constexpr (sizeof(T) == 4) return r[k];
    else return (uint32_t)(r[k >> 1] >> (32 * (k & 1)));
}

template <typename T, int FX, int ZEROS>
__global__ __launch_bounds__(LBD_T) void downsample_box_labels_kernel(const T* __restrict__ win, BoxGeom g, DsPlan p,
                                                                      T* __restrict__ out) {
    constexpr int P = LBD_PIECE / (int)sizeof(T);
    constexpr int OUTS = P / FX;
    const int bx1 = g.b0[2] + g.bd[2];
    // source x that may be read: the box's, cut at the volume (the window holds them: checked on the host)
    const int sx0 = g.b0[2] * FX, sx1 = min(g.n[2], bx1 * FX);
    for (int z = g.b0[0] + (int)blockIdx.z; z < g.b0[0] + g.bd[0]; z += (int)gridDim.z) {
        for (int y = g.b0[1] + (int)(blockIdx.y * blockDim.y + threadIdx.y); y < g.b0[1] + g.bd[1];
             y += (int)(gridDim.y * blockDim.y)) {
            // the source rows; a row past the volume, or of a factor of 1, repeats the one before it
            const T* rows[2][2];
#pragma unroll
            for (int dz = 0; dz < 2; dz++) {
#pragma unroll
                for (int dy = 0; dy < 2; dy++) {
                    const int zs = min(z * p.f[0] + (dz & (p.f[0] - 1)), g.n[0] - 1);
                    const int ys = min(y * p.f[1] + (dy & (p.f[1] - 1)), g.n[1] - 1);
                    rows[dz][dy] = win + ((size_t)(zs - g.w0[0]) * g.wd[1] + (size_t)(ys - g.w0[1])) * (size_t)g.wd[2];
                }
            }
            T* orow = out + ((size_t)(z - g.b0[0]) * g.bd[1] + (size_t)(y - g.b0[1])) * (size_t)g.bd[2];
            for (int pc = (int)(blockIdx.x * blockDim.x + threadIdx.x); pc < p.pieces; pc += (int)(gridDim.x * blockDim.x)) {
                const int xo = p.ox + pc * OUTS;                 // the piece's first output x (level)
                const int xs = xo * FX;                          // and its first source x
                uint32_t ok = 0;                                 // per element: a voxel of the box's source
#pragma unroll
                for (int e = 0; e < P; e++)
                    if (xs + e >= sx0 && xs + e < sx1) ok |= 1u << e;
                const bool vec = p.vec_in && xs >= g.w0[2] && xs + P <= g.w0[2] + g.wd[2];
                T d[2][2][P];
#pragma unroll
                for (int dz = 0; dz < 2; dz++) {
#pragma unroll
                    for (int dy = 0; dy < 2; dy++) {
                        // a repeated row is copied in registers, not read again: fz fy rows are read per piece
                        const bool same_z = dz && rows[dz][dy] == rows[0][dy];
                        const bool same_y = dy && rows[dz][dy] == rows[dz][0];
                        if (same_z || same_y) {
#pragma unroll
                            for (int q = 0; q < P; q++) d[dz][dy][q] = same_z ? d[0][dy][q] : d[dz][0][q];
                            continue;
                        }
                        const T* src = rows[dz][dy] + (xs - g.w0[2]);
                        if (vec) {
                            const uint4 v = *reinterpret_cast<const uint4*>(src);
                            if constexpr (sizeof(T) == 4) {
                                d[dz][dy][0] = v.x; d[dz][dy][1] = v.y; d[dz][dy][2] = v.z; d[dz][dy][3] = v.w;
                            } else {
                                d[dz][dy][0] = (T)v.x | (T)v.y << 32;
                                d[dz][dy][1] = (T)v.z | (T)v.w << 32;
                            }
                        } else {
#pragma unroll
                            for (int e = 0; e < P; e++) d[dz][dy][e] = (ok >> e & 1u) ? src[e] : (T)0;
                        }
                    }
                }
                T r[OUTS];
#pragma unroll
                for (int j = 0; j < OUTS; j++) {
                    if constexpr (FX == 2) {
                        T v[8];
                        const bool second = ok >> (2 * j + 1) & 1u;      // else x is cut: repeat the first voxel
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            v[2 * k] = d[k >> 1][k & 1][2 * j];
                            v[2 * k + 1] = second ? d[k >> 1][k & 1][2 * j + 1] : d[k >> 1][k & 1][2 * j];
                        }
                        r[j] = label_mode<ZEROS>(v);
                    } else {
                        T v[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) v[k] = d[k >> 1][k & 1][j];
                        r[j] = label_mode<ZEROS>(v);
                    }
                }
                T* dst = orow + (xo - g.b0[2]);
                if (p.vec_out && xo >= g.b0[2] && xo + OUTS <= bx1) {
                    if constexpr (OUTS * sizeof(T) == 16) {
                        uint4 v;
                        v.x = label_word(r, 0); v.y = label_word(r, 1); v.z = label_word(r, 2); v.w = label_word(r, 3);
                        *reinterpret_cast<uint4*>(dst) = v;
                    } else {
                        static_assert(OUTS * sizeof(T) == 8, "a piece stores 8 or 16 bytes");
                        uint2 v;
                        v.x = label_word(r, 0); v.y = label_word(r, 1);
                        *reinterpret_cast<uint2*>(dst) = v;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < OUTS; j++)
                        if (xo + j >= g.b0[2] && xo + j < bx1) dst[j] = r[j];
                }
            }
        }
    }
}

void label_downsample_box_plan(const void* win, int typesize, const BoxGeom& g, const int* factors, const void* out,
                               DsPlan& p) {
    for (int a = 0; a < 3; a++) p.f[a] = factors[a];
    const int per = LBD_PIECE / typesize;             // voxels of a piece
    const int fx = factors[2], outs = per / fx;
    // the element of the window's allocation (mod per) at which the box's first source voxel of every row lies
    const int phase = (int)(((uintptr_t)win / (uintptr_t)typesize + (uintptr_t)(g.b0[2] * fx - g.w0[2])) &
                            (uintptr_t)(per - 1));
    const bool pitch_out = g.bd[2] % outs == 0;
    const int out_phase = (int)(((uintptr_t)out / (uintptr_t)typesize) & (uintptr_t)(outs - 1));
    int oshift;
    p.vec_in = g.wd[2] % per == 0 && phase % fx == 0;
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
    p.block[1] = (unsigned)(LBD_T / bx);
    p.grid[0] = (unsigned)((p.pieces + bx - 1) / bx);
    p.grid[1] = (unsigned)std::min<long long>(((long long)g.bd[1] + p.block[1] - 1) / p.block[1], 65535);
    p.grid[2] = (unsigned)std::min(g.bd[0], 65535);
}

template <typename T>
static hipError_t launch_labels_t(const T* win, const BoxGeom& g, const DsPlan& p, int zeros, T* out, hipStream_t s) {
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block[0], p.block[1]);
#define LBD_LAUNCH(FX, Z) hipLaunchKernelGGL((downsample_box_labels_kernel<T, FX, Z>), grid, block, 0, s, win, g, p, out)
    if (p.f[2] == 2) {
        if (zeros == LABEL_ZEROS_IGNORE) LBD_LAUNCH(2, LABEL_ZEROS_IGNORE);
        else LBD_LAUNCH(2, LABEL_ZEROS_COUNT);
    } else {
        if (zeros == LABEL_ZEROS_IGNORE) LBD_LAUNCH(1, LABEL_ZEROS_IGNORE);
        else LBD_LAUNCH(1, LABEL_ZEROS_COUNT);
    }
#undef LBD_LAUNCH
    return hipGetLastError();
}

hipError_t launch_downsample_box_labels(const void* win, int typesize, const BoxGeom& g, const DsPlan& p, int zeros,
                                        void* out, hipStream_t s) {
    if (typesize == 4)
        return launch_labels_t(static_cast<const uint32_t*>(win), g, p, zeros, static_cast<uint32_t*>(out), s);
    return launch_labels_t(static_cast<const uint64_t*>(win), g, p, zeros, static_cast<uint64_t*>(out), s);
}

}  // namespace exabm4d
