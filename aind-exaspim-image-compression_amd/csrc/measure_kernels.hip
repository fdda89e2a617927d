// measure_kernels.hip -- measuring a stored volume brick by brick: one pass over a box
// inside a window (BoxGeom, exabm4d_kernels.h) ADDS to two integer tables resident on the device,
//
//   counts[v] += 1                      for every voxel of the box (the exact histogram of the uint16 counts), and
//   wide[level(s)][wide_bin(|d|)] += 1, sum_s[level(s)] += s
//                                       for every 2x2x2 cell of the VOLUME'S even grid whose origin lies in the box,
//
// with s, d and the level those of noise_kernels.hip (noise_cell.h).  A cell is counted by the box that holds its
// origin, so boxes may begin and end at odd coordinates and any partition of a volume counts every cell once; the
// far corner of such a cell may lie one voxel outside the box, inside the window (the host layer checks that).
//
// The wide bin keeps |d| = m < 2^18 exactly below 4096 and to 11 significant bits above it, octave by octave:
//   m < 4096: bin m;  otherwise j = floor(log2 m) - 11 (1..6), bin 4096 + (j - 1) 2048 + ((m >> j) - 2048).
// Every bin lies inside one bin of the table at any shift 0..6 (octave j is at least as fine as 2^k for j <= k, and
// holds only m >= 4096 << k for j > k, the last bin), so the host folds one wide table into the table of any shift
// exactly: the volume is read once where the in-memory rule repeats its pass.
//
// With a mask window (non-zero = foreground) both tables come twice, foreground then background: a voxel counts in
// the table its mask names, a cell is background only if all eight of its voxels are.
//
// All counters are integers: the tables depend neither on the launch nor on how the volume was cut into boxes.
#include "exabm4d_kernels.h"
#include "noise_cell.h"

namespace exabm4d {

// LDS.  ExaSPIM volumes are mostly background: nearly every voxel has one of a few hundred low values, nearly every
// cell falls into two or three levels and a few hundred bins, and global atomics on those addresses would
// serialise.  A workgroup therefore keeps, as 32-bit counters,
//   * MS_SLOTS rows of the wide table's first 4096 bins (the bins >= 4096 are |d| >= 4096: structure, not noise, and
//     rare), direct-mapped by (level * tables + table) % MS_SLOTS and tagged with the row that claimed the slot
//     first, as noise_table_kernel does it: six slots hold three adjacent levels of both tables, or six adjacent
//     levels without a mask;
//   * the first MS_BAND / tables values of each counts table, as diff_hist_kernel keeps its band;
// and the per-level sums of s as 64-bit counters in MS_COLS columns.  6 * 16 KiB + 32 KiB + 2 * 49 * 16 * 8 B is
// 140.3 KiB of the CU's 160: one workgroup of 1024 per CU, which flushes its non-zero counters once, at its end.
// Everything else -- a wide bin >= 4096, a row that lost its slot, a value beyond the band -- is a 64-bit global
// atomic at once.  noise_table_kernel's eight slots alone take 128 KiB; six leave room for the counts band, and two
// tables of three levels each is what a masked background needs.
constexpr int MS_T = 1024;
constexpr int MS_SLOTS = 6;
constexpr int MS_COLS = 16;
constexpr int MS_BAND = 8192;
constexpr size_t ms_lds_bytes(int tables) {
    return (size_t)tables * NOISE_LEVELS * MS_COLS * 8 + (size_t)MS_SLOTS * NOISE_BINS * 4 + (size_t)MS_BAND * 4 + 64;
}

__device__ __forceinline__ uint32_t noise_wide_bin(uint32_t m) {      // m <= 4 * 65535
    if (m < (uint32_t)NOISE_BINS) return m;
    const int j = (31 - __clz(m)) - 11;                                // 1 .. 6
    return (uint32_t)NOISE_BINS + (uint32_t)(j - 1) * 2048u + ((m >> j) - 2048u);
}

template <int TABLES>
struct MeasureLds {
    static constexpr int BAND = MS_BAND / TABLES;
    static constexpr size_t NOISE_STRIDE = (size_t)NOISE_LEVELS * NOISE_WIDE_BINS + NOISE_LEVELS;
    unsigned long long* sums;   // [TABLES][NOISE_LEVELS][MS_COLS]
    uint32_t* bins;             // [MS_SLOTS][NOISE_BINS]
    uint32_t* band;             // [TABLES][BAND]
    volatile int* tags;         // [MS_SLOTS]: level * TABLES + table of the row a slot holds, -1 = free

    __device__ __forceinline__ void voxel(uint32_t v, int t, unsigned long long* __restrict__ counts) const {
        if (v < (uint32_t)BAND) atomicAdd(&band[t * BAND + (int)v], 1u);
        else atomicAdd(&counts[(size_t)t * COUNT_BINS + v], 1ull);
    }

    __device__ __forceinline__ void cell(uint32_t s, uint32_t m, int t, unsigned long long* __restrict__ noise) const {
        const int lv = noise_level(s);
        const uint32_t w = noise_wide_bin(m);
        atomicAdd(&sums[(t * NOISE_LEVELS + lv) * MS_COLS + (threadIdx.x & (MS_COLS - 1))], (unsigned long long)s);
        unsigned long long* row = noise + (size_t)t * NOISE_STRIDE + (size_t)lv * NOISE_WIDE_BINS;
        if (w >= (uint32_t)NOISE_BINS) {
            atomicAdd(&row[w], 1ull);
            return;
        }
        const int want = lv * TABLES + t;
        const int slot = want % MS_SLOTS;
        int tag = tags[slot];
        if (tag < 0) {
            tag = atomicCAS(const_cast<int*>(&tags[slot]), -1, want);
            if (tag < 0) tag = want;
        }
        if (tag == want) atomicAdd(&bins[slot * NOISE_BINS + (int)w], 1u);
        else atomicAdd(&row[w], 1ull);
    }
};

// Eight voxels xg .. xg + 7 (volume coordinates, xg even) of the row (z, y) as four dwords; what lies outside the
// window reads 0 and is never counted.  vec: the 16 bytes are aligned and the caller's phase makes xg - w0x a
// multiple of 8 elements from an aligned row start, so a group wholly inside the window's row is one vector load.
__device__ __forceinline__ void load_row8(const uint16_t* __restrict__ win, const BoxGeom& g, int z, int y, int xg,
                                          bool vec, uint32_t (&d)[4]) {
    d[0] = d[1] = d[2] = d[3] = 0u;
    if (z < g.w0[0] || z >= g.w0[0] + g.wd[0] || y < g.w0[1] || y >= g.w0[1] + g.wd[1]) return;
    const uint16_t* row = win + ((size_t)(z - g.w0[0]) * g.wd[1] + (size_t)(y - g.w0[1])) * (size_t)g.wd[2];
    const int xo = xg - g.w0[2];
    if (vec && xo >= 0 && xo + 8 <= g.wd[2]) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + xo);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int x = xo + e;
        if (x >= 0 && x < g.wd[2]) d[e >> 1] |= (uint32_t)row[x] << ((e & 1) * 16);
    }
}

// Work items: a pair of cell rows (zc, yc) -- the rows (2 zc, 2 zc + 1) x (2 yc, 2 yc + 1) of the volume that meet
// the box -- times a group of eight x starting at xs + 8 v.  lx = tid & (LX - 1) walks the groups of a pair of rows,
// tid >> lx_log2 picks one of MS_T / LX pairs; pairs are dealt to the workgroups round-robin (noise_table_kernel's
// scheme).  A lane counts the voxels of its 4 x 8 that lie in the box and the up to four cells whose origins do.
template <int TABLES>
__global__ __launch_bounds__(MS_T) void measure_box_kernel(const uint16_t* __restrict__ win,
                                                           const uint16_t* __restrict__ mask, BoxGeom g, int vector_ok,
                                                           int xs, int ngx, int lx_log2,
                                                           unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ noise) {
    extern __shared__ unsigned long long ms_lds[];
    using L_t = MeasureLds<TABLES>;
    L_t L;
    L.sums = ms_lds;
    L.bins = reinterpret_cast<uint32_t*>(ms_lds + TABLES * NOISE_LEVELS * MS_COLS);
    L.band = L.bins + MS_SLOTS * NOISE_BINS;
    int* tags = reinterpret_cast<int*>(L.band + MS_BAND);
    L.tags = tags;
    const int tid = threadIdx.x;
    for (int i = tid; i < TABLES * NOISE_LEVELS * MS_COLS; i += MS_T) L.sums[i] = 0ull;
    for (int i = tid; i < MS_SLOTS * NOISE_BINS + MS_BAND; i += MS_T) L.bins[i] = 0u;     // the band follows the bins
    if (tid < MS_SLOTS) tags[tid] = -1;
    __syncthreads();

    const int bz0 = g.b0[0], bz1 = g.b0[0] + g.bd[0], by0 = g.b0[1], by1 = g.b0[1] + g.bd[1];
    const int bx0 = g.b0[2], bx1 = g.b0[2] + g.bd[2];
    const int ez = g.n[0] & ~1, ey = g.n[1] & ~1, ex = g.n[2] & ~1;      // cell origins lie below these
    const int zc0 = bz0 >> 1, yc0 = by0 >> 1;
    const uint32_t cy = (uint32_t)(((by1 - 1) >> 1) - yc0 + 1);
    const uint32_t npr = (uint32_t)(((bz1 - 1) >> 1) - zc0 + 1) * cy;    // < 2^31 (checked by the launcher)
    const int LX = 1 << lx_log2;
    const int lx = tid & (LX - 1);
    const uint32_t rows_per_wg = (uint32_t)(MS_T >> lx_log2);
    const bool vec = vector_ok != 0;
    for (uint32_t pr = blockIdx.x * rows_per_wg + (uint32_t)(tid >> lx_log2); pr < npr;
         pr += gridDim.x * rows_per_wg) {
        const uint32_t zi = pr / cy;
        const int z = 2 * (zc0 + (int)zi), y = 2 * (yc0 + (int)(pr - zi * cy));
        bool row_in[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int zz = z + (r >> 1), yy = y + (r & 1);
            row_in[r] = zz >= bz0 && zz < bz1 && yy >= by0 && yy < by1;
        }
        const bool cell_zy = row_in[0] && z < ez && y < ey;              // the origin's row is in the box
        for (int v = lx; v < ngx; v += LX) {
            const int xg = xs + 8 * v;
            uint32_t d[4][4], k[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int zz = z + (r >> 1), yy = y + (r & 1);
                if (row_in[r] || cell_zy) {
                    load_row8(win, g, zz, yy, xg, vec, d[r]);
                    if (TABLES == 2) load_row8(mask, g, zz, yy, xg, vec, k[r]);
                } else {
                    d[r][0] = d[r][1] = d[r][2] = d[r][3] = 0u;
                    k[r][0] = k[r][1] = k[r][2] = k[r][3] = 0u;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if (!row_in[r]) continue;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int x = xg + e;
                    if (x < bx0 || x >= bx1) continue;
                    const uint32_t val = (d[r][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
                    int t = 0;
                    if (TABLES == 2) t = ((k[r][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu) ? 0 : 1;
                    L.voxel(val, t, counts);
                }
            }
            if (!cell_zy) continue;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int x = xg + 2 * c;
                if (x < bx0 || x >= bx1 || x >= ex) continue;
                uint32_t s, m;
                cell_u16_sm(d[0][c], d[1][c], d[2][c], d[3][c], s, m);
                int t = 0;
                if (TABLES == 2) t = (k[0][c] | k[1][c] | k[2][c] | k[3][c]) ? 0 : 1;
                L.cell(s, m, t, noise);
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < MS_BAND; i += MS_T) {
        const uint32_t c = L.band[i];
        if (c) atomicAdd(&counts[(size_t)(i / L_t::BAND) * COUNT_BINS + (size_t)(i % L_t::BAND)], (unsigned long long)c);
    }
    for (int slot = 0; slot < MS_SLOTS; slot++) {
        const int tag = tags[slot];
        if (tag < 0) continue;
        unsigned long long* row = noise + (size_t)(tag % TABLES) * L_t::NOISE_STRIDE +
                                  (size_t)(tag / TABLES) * NOISE_WIDE_BINS;
        for (int i = tid; i < NOISE_BINS; i += MS_T) {
            const uint32_t c = L.bins[slot * NOISE_BINS + i];
            if (c) atomicAdd(&row[i], (unsigned long long)c);
        }
    }
    if (tid < TABLES * NOISE_LEVELS) {
        unsigned long long t = 0ull;
        for (int c = 0; c < MS_COLS; c++) t += L.sums[tid * MS_COLS + c];
        if (t)
            atomicAdd(&noise[(size_t)(tid / NOISE_LEVELS) * L_t::NOISE_STRIDE + (size_t)NOISE_LEVELS * NOISE_WIDE_BINS +
                             (size_t)(tid % NOISE_LEVELS)], t);
    }
}

size_t measure_counts_bytes(int tables) { return (size_t)tables * COUNT_BINS * sizeof(unsigned long long); }
size_t measure_noise_bytes(int tables) {
    return (size_t)tables * ((size_t)NOISE_LEVELS * NOISE_WIDE_BINS + NOISE_LEVELS) * sizeof(unsigned long long);
}

hipError_t measure_prepare(int device, int* wgs) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&measure_box_kernel<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)ms_lds_bytes(1));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&measure_box_kernel<2>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)ms_lds_bytes(2));
    if (e != hipSuccess) return e;
    int cus = 0;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return e;
    *wgs = cus > 0 ? cus : 1;
    return hipSuccess;
}

bool measure_box_plan(const uint16_t* win, const uint16_t* mask, const BoxGeom& g, int wgs, MeasurePlan& p) {
    // 16-byte loads: both windows at one phase of 16 bytes, a pitch of whole vectors, and groups of eight that begin
    // at an even x (a cell's) -- x = w0x - (phase in elements) mod 8 -- which an odd phase does not give
    const int phase = (int)(((uintptr_t)win >> 1) & 7u);
    const int first = (g.w0[2] - phase) & 7;         // the x (mod 8) at which vectors of a row are aligned
    p.vector_ok = g.wd[2] % 8 == 0 && (first & 1) == 0 && (!mask || (int)(((uintptr_t)mask >> 1) & 7u) == phase);
    p.xs = g.b0[2] & ~1;
    if (p.vector_ok) p.xs -= (p.xs - first) & 7;     // the last aligned x at or below it; may lie below the window
    const int x_end = (g.b0[2] + g.bd[2] + 1) & ~1;  // the box and the far column of its last cell
    p.ngx = (x_end - p.xs + 7) / 8;
    p.lx_log2 = 0;
    while ((1 << p.lx_log2) < p.ngx && (1 << p.lx_log2) < MS_T) p.lx_log2++;
    const long long rows_per_wg = MS_T >> p.lx_log2;
    const long long npr = (long long)(((g.b0[0] + g.bd[0] - 1) >> 1) - (g.b0[0] >> 1) + 1) *
                          (long long)(((g.b0[1] + g.bd[1] - 1) >> 1) - (g.b0[1] >> 1) + 1);
    if (npr >= (1ll << 31)) return false;
    long long blocks = (npr + rows_per_wg - 1) / rows_per_wg;
    if (blocks > (wgs > 0 ? wgs : 1)) blocks = wgs > 0 ? wgs : 1;
    p.blocks = (unsigned)blocks;
    // a workgroup's 32-bit counters: its share of the pairs of rows holds fewer than 2^32 voxels
    const long long rounds = (npr + blocks * rows_per_wg - 1) / (blocks * rows_per_wg);
    return rounds * rows_per_wg * 4 * 8 * (long long)p.ngx < (1ll << 32);
}

hipError_t launch_measure_box_u16(const uint16_t* win, const uint16_t* mask, const BoxGeom& g, const MeasurePlan& p,
                                  unsigned long long* counts, unsigned long long* noise, hipStream_t s) {
    if (mask)
        hipLaunchKernelGGL(measure_box_kernel<2>, dim3(p.blocks), dim3(MS_T), ms_lds_bytes(2), s, win, mask, g,
                           p.vector_ok, p.xs, p.ngx, p.lx_log2, counts, noise);
    else
        hipLaunchKernelGGL(measure_box_kernel<1>, dim3(p.blocks), dim3(MS_T), ms_lds_bytes(1), s, win, mask, g,
                           p.vector_ok, p.xs, p.ngx, p.lx_log2, counts, noise);
    return hipGetLastError();
}

}  // namespace exabm4d
