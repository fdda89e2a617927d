// compare_kernels.hip -- scoring one stored volume against another brick by brick.
//
// Every operation works on a box inside a window (BoxGeom, exabm4d_kernels.h): one region read of a brick and
// its SSIM halo serves all of them.
//
//   diff_hist_kernel   the signed difference table hist[(test - ref) + 65535] += 1, split by a mask window
//                      when there is one: MAE, MSE, bias, the maximum and every percentile of the error follow
//                      from it on the host in integer arithmetic, whatever the brick plan was.
//   mip3_kernel        the maxima over z, y and x of ref, test and |test - ref| over the box, folded into
//                      nine planes of the whole volume's extents.
//   (SSIM of a box)    ssim3d_kernel of metrics_kernels.hip, whose index arithmetic takes the same BoxGeom.
//
// All counters and maxima are integers: neither result depends on the launch shape, the order in which
// workgroups retire or the bricks a caller cuts.
#include "exabm4d_kernels.h"

namespace exabm4d {

// ---- signed difference histogram --------------------------------------------------------------------------------
// 131071 bins of 4 bytes are 512 KiB, the LDS has 160 KiB.  The band kept in LDS is the DH_BAND = 4096 bins of the
// differences -2048 .. 2047, as 32-bit counters: 16 KiB a table, 32 KiB with a mask.  Why that band: the error of a
// denoised or a bounded lossy volume is the noise that was removed or the codec's bound -- tens of counts, a few
// hundred on the brightest neurites (shot noise of 10^4 counts is 100) -- so 2048 either side takes all but stray
// voxels, while 32 KiB still leaves room for four or five workgroups of 256 on a CU to hide the loads' latency
// (a band of 16384 bins would take that down to one).  A workgroup counts its voxels' differences inside the band
// with LDS atomics and adds every non-zero bin to the table once, at its end; a difference outside the band goes
// to the table at once with a 64-bit atomic.  Full-range data (differences of +-65535) is therefore correct and
// runs at the rate of global atomics.  A workgroup takes fewer than 2^31 voxels (box <= 2^40 voxels over up to
// DH_MAX_WGS workgroups, in steps of at most max(DH_STEP, bx) voxels), so no 32-bit counter can wrap.
constexpr int DH_T = 256;
constexpr int DH_BAND = 4096;
constexpr int DH_HALF = DH_BAND / 2;
constexpr int DH_STEP = 8192;        // voxels of whole box rows a workgroup takes at a time
constexpr int DH_MAX_WGS = 2048;     // 8 per CU

template <bool MASK>
__global__ __launch_bounds__(DH_T) void diff_hist_kernel(const uint16_t* __restrict__ ref,
                                                         const uint16_t* __restrict__ test,
                                                         const uint16_t* __restrict__ mask, BoxGeom g, int rows_per_step,
                                                         unsigned long long* __restrict__ hist) {
    constexpr int TABLES = MASK ? 2 : 1;
    __shared__ uint32_t band[TABLES * DH_BAND];
    const int tid = threadIdx.x;
    for (int i = tid; i < TABLES * DH_BAND; i += DH_T) band[i] = 0u;
    __syncthreads();
    const int by = g.bd[1], bx = g.bd[2];
    const long long rows = (long long)g.bd[0] * by;
    const long long steps = (rows + rows_per_step - 1) / rows_per_step;
    const size_t sy = (size_t)g.wd[2], sz = (size_t)g.wd[1] * g.wd[2];
    const size_t base = (size_t)(g.b0[0] - g.w0[0]) * sz + (size_t)(g.b0[1] - g.w0[1]) * sy + (size_t)(g.b0[2] - g.w0[2]);
    for (long long st = blockIdx.x; st < steps; st += gridDim.x) {
        const long long row0 = st * rows_per_step;
        const long long left = rows - row0;
        const int nrows = left < rows_per_step ? (int)left : rows_per_step;
        const int z0 = (int)(row0 / by), y0 = (int)(row0 - (long long)z0 * by);
        const int nel = nrows * bx;
        for (int e = tid; e < nel; e += DH_T) {
            const int r = e / bx, x = e - r * bx;
            const int yy = y0 + r, dz = yy / by, y = yy - dz * by;
            const size_t i = base + (size_t)(z0 + dz) * sz + (size_t)y * sy + (size_t)x;
            const int d = (int)test[i] - (int)ref[i];
            int t = 0;
            if (MASK) t = mask[i] != 0 ? 0 : 1;      // table 0: foreground, table 1: background
            const unsigned c = (unsigned)(d + DH_HALF);
            if (c < (unsigned)DH_BAND)
                atomicAdd(&band[t * DH_BAND + (int)c], 1u);
            else
                atomicAdd(&hist[(size_t)t * DIFF_BINS + (size_t)(d + 65535)], 1ull);
        }
    }
    __syncthreads();
    for (int i = tid; i < TABLES * DH_BAND; i += DH_T) {
        const uint32_t c = band[i];
        if (c) {
            const int t = i / DH_BAND, b = i - t * DH_BAND;
            atomicAdd(&hist[(size_t)t * DIFF_BINS + (size_t)(b - DH_HALF + 65535)], (unsigned long long)c);
        }
    }
}

hipError_t launch_diff_hist_u16(const uint16_t* ref, const uint16_t* test, const uint16_t* mask, const BoxGeom& g,
                                unsigned long long* hist, hipStream_t s) {
    const int rows_per_step = std::max(1, DH_STEP / g.bd[2]);
    const long long rows = (long long)g.bd[0] * g.bd[1];
    const long long steps = (rows + rows_per_step - 1) / rows_per_step;
    const unsigned blocks = (unsigned)std::min<long long>(steps, DH_MAX_WGS);
    if (mask)
        hipLaunchKernelGGL(diff_hist_kernel<true>, dim3(blocks), dim3(DH_T), 0, s, ref, test, mask, g, rows_per_step,
                           hist);
    else
        hipLaunchKernelGGL(diff_hist_kernel<false>, dim3(blocks), dim3(DH_T), 0, s, ref, test, mask, g, rows_per_step,
                           hist);
    return hipGetLastError();
}

// ---- three-axis maximum projections -----------------------------------------------------------------------------
// One workgroup owns MP_TY (y) x MP_TX (x) columns of the box over MP_ZC layers; wave q holds the rows q, q + 4,
// q + 8, q + 12 of the tile, a lane one x.  The three reductions happen on chip before anything leaves it:
//   over z  in registers while the workgroup walks its layers: one atomic per column at the end;
//   over x  across the 64 lanes of a wave (a row of the tile): one atomic per row and layer, by lane 0;
//   over y  of the four rows a lane holds in registers, then of the four waves with LDS atomics into a
//           [layer][volume][x] table: one atomic per x and layer at the end.
// That leaves 3/32 + 3/64 + 3/16 global atomics a voxel, and none for a zero (the planes start at zero and zero is
// max's identity).  The planes are 32-bit words: the device has no 16-bit atomic maximum.
constexpr int MP_T = 256;
constexpr int MP_TX = 64;
constexpr int MP_TY = 16;
constexpr int MP_ZC = 32;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

__global__ __launch_bounds__(MP_T) void mip3_kernel(const uint16_t* __restrict__ ref,
                                                    const uint16_t* __restrict__ test, BoxGeom g,
                                                    uint32_t* __restrict__ planes) {
    __shared__ uint32_t zx[MP_ZC * 3 * MP_TX];
    const int tid = threadIdx.x;
    for (int i = tid; i < MP_ZC * 3 * MP_TX; i += MP_T) zx[i] = 0u;
    __syncthreads();
    const int nz = g.n[0], ny = g.n[1], nx = g.n[2];
    const int bz = g.bd[0], by = g.bd[1], bx = g.bd[2];
    const int tiles_x = (bx + MP_TX - 1) / MP_TX, tiles_y = (by + MP_TY - 1) / MP_TY;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const int tz = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = tx * MP_TX, y0 = ty * MP_TY, zs = tz * MP_ZC, ze = min(bz, zs + MP_ZC);   // inside the box
    const int ox = tid & 63, oy = tid >> 6;
    const int x = x0 + ox;
    const bool xin = x < bx;
    const size_t sy = (size_t)g.wd[2], sz = (size_t)g.wd[1] * g.wd[2];
    const size_t base = (size_t)(g.b0[0] - g.w0[0]) * sz + (size_t)(g.b0[1] - g.w0[1]) * sy + (size_t)(g.b0[2] - g.w0[2]);
    const size_t n_yx = (size_t)ny * nx, n_zx = (size_t)nz * nx, words = n_yx + n_zx + (size_t)nz * ny;
    uint32_t col[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++) col[j][0] = col[j][1] = col[j][2] = 0u;

    for (int z = zs; z < ze; z++) {
        uint32_t rx[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int y = y0 + oy + 4 * j;      // the same for the whole wave
            uint32_t v[3] = {0u, 0u, 0u};
            if (xin && y < by) {
                const size_t i = base + (size_t)z * sz + (size_t)y * sy + (size_t)x;
                v[0] = ref[i];
                v[1] = test[i];
                v[2] = v[0] > v[1] ? v[0] - v[1] : v[1] - v[0];
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                col[j][q] = max(col[j][q], v[q]);
                rx[q] = max(rx[q], v[q]);
                const uint32_t m = wave_max_u32(v[q]);
                if (ox == 0 && y < by && m)
                    atomicMax(&planes[q * words + n_yx + n_zx + (size_t)(g.b0[0] + z) * ny + (size_t)(g.b0[1] + y)], m);
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++)
            if (rx[q]) atomicMax(&zx[((z - zs) * 3 + q) * MP_TX + ox], rx[q]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + oy + 4 * j;
        if (xin && y < by) {
            const size_t o = (size_t)(g.b0[1] + y) * nx + (size_t)(g.b0[2] + x);
#pragma unroll
            for (int q = 0; q < 3; q++)
                if (col[j][q]) atomicMax(&planes[q * words + o], col[j][q]);
        }
    }
    __syncthreads();
    for (int i = tid; i < (ze - zs) * 3 * MP_TX; i += MP_T) {
        const uint32_t m = zx[i];
        const int xx = i % MP_TX, q = (i / MP_TX) % 3, zi = i / (3 * MP_TX);
        if (m && x0 + xx < bx)
            atomicMax(&planes[q * words + n_yx + (size_t)(g.b0[0] + zs + zi) * nx + (size_t)(g.b0[2] + x0 + xx)], m);
    }
}

size_t mip3_plane_words(const BoxGeom& g) {
    return (size_t)g.n[1] * g.n[2] + (size_t)g.n[0] * g.n[2] + (size_t)g.n[0] * g.n[1];
}

hipError_t launch_mip3_u16(const uint16_t* ref, const uint16_t* test, const BoxGeom& g, uint32_t* planes,
                           hipStream_t s) {
    const long long blocks = (long long)((g.bd[2] + MP_TX - 1) / MP_TX) * ((g.bd[1] + MP_TY - 1) / MP_TY) *
                             ((g.bd[0] + MP_ZC - 1) / MP_ZC);
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mip3_kernel, dim3((unsigned)blocks), dim3(MP_T), 0, s, ref, test, g, planes);
    return hipGetLastError();
}

}  // namespace exabm4d
