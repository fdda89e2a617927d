// noise_kernels.hip -- the noise table: one pass over a volume resident in HBM (gfx950).
//
// The volume is cut into 2x2x2 cells at even coordinates.  Every cell gives s = sum of its eight voxels and
// d = sum of (-1)^(dz+dy+dx) v, the unnormalised Haar HHH detail: two orthogonal combinations, so for i.i.d.
// noise Var d = 8 sigma^2 and d does not depend on the cell mean.  The cell is counted in
// hist[level(s)][min(|d| >> shift, NOISE_BINS - 1)], level = the quarter-octave bin of the cell mean, and s is
// added to sum_s[level].  The median of a row of the table is a robust noise sigma at that intensity; the
// estimators on top of it are host scalar work (utils/noise.py).
//
// All counters are integers: the table does not depend on the launch shape or the order of the updates.
#include "exabm4d_kernels.h"
#include "noise_cell.h"

namespace exabm4d {

// ExaSPIM volumes are mostly background: nearly all cells fall into two or three levels and a few hundred
// bins, and global atomics on those addresses would serialise.  A workgroup keeps NT_SLOTS rows of the table
// as 32-bit counters in LDS (8 * 4096 * 4 B = 128 KB), direct-mapped by level & 7 and tagged with the level
// that claimed the slot first; a cell whose level lost its slot to another goes to a 64-bit global atomic.
// The per-level sums of s sit beside them as 64-bit LDS counters, NT_COLS columns per level so that the lanes
// of a wave do not all add to one address.  A workgroup flushes its non-zero counters once, when it is done.
constexpr int NT_T = 1024;
constexpr int NT_SLOTS = 8;
constexpr int NT_COLS = 32;
constexpr size_t NT_LDS = (size_t)NOISE_LEVELS * NT_COLS * 8 + (size_t)NT_SLOTS * NOISE_BINS * 4 + 64;
constexpr uint32_t NT_S_MAX = 8u * 65535u;

struct NoiseLds {
    unsigned long long* sums;   // [NOISE_LEVELS][NT_COLS]
    uint32_t* bins;             // [NT_SLOTS][NOISE_BINS]
    volatile int* tags;         // [NT_SLOTS]: the level a slot holds, -1 = free
    uint32_t* skipped;

    // s <= NT_S_MAX; m = |d|, anything >= NOISE_BINS << shift lands in the last bin
    __device__ __forceinline__ void count(uint32_t s, uint32_t m, int shift,
                                          unsigned long long* __restrict__ hist) const {
        const int lv = noise_level(s);
        const uint32_t b = min(m >> shift, (uint32_t)(NOISE_BINS - 1));
        atomicAdd(&sums[lv * NT_COLS + (threadIdx.x & (NT_COLS - 1))], (unsigned long long)s);
        const int slot = lv & (NT_SLOTS - 1);
        int tag = tags[slot];
        if (tag < 0) {
            tag = atomicCAS(const_cast<int*>(&tags[slot]), -1, lv);
            if (tag < 0) tag = lv;
        }
        if (tag == lv) atomicAdd(&bins[slot * NOISE_BINS + b], 1u);
        else atomicAdd(&hist[(size_t)lv * NOISE_BINS + b], 1ull);
    }
};

// One cell of uint16 voxels (cell_u16_sm of noise_cell.h names the four dwords).
__device__ __forceinline__ void cell_u16(const NoiseLds& L, uint32_t a, uint32_t b, uint32_t c, uint32_t d, int shift,
                                         unsigned long long* __restrict__ hist) {
    uint32_t s, m;
    cell_u16_sm(a, b, c, d, s, m);
    L.count(s, m, shift, hist);
}

// One cell of fp32 voxels v[dz][dy][dx], with the association the specification fixes.
__device__ __forceinline__ void cell_f32(const NoiseLds& L, float v000, float v001, float v010, float v011, float v100,
                                         float v101, float v110, float v111, int shift,
                                         unsigned long long* __restrict__ hist) {
    const float s = ((v000 + v001) + (v010 + v011)) + ((v100 + v101) + (v110 + v111));
    const float d = ((v000 - v001) - (v010 - v011)) - ((v100 - v101) - (v110 - v111));
    if (!(isfinite(s) && isfinite(d))) {
        atomicAdd(L.skipped, 1u);
        return;
    }
    const float sf = fminf(fmaxf(floorf(s), 0.0f), (float)NT_S_MAX);
    const float ad = fabsf(d);
    const uint32_t m = ad >= 16777216.0f ? 0xFFFFFFFFu : (uint32_t)rintf(ad);   // rintf: half to even
    L.count((uint32_t)sf, m, shift, hist);
}

__device__ __forceinline__ float as_f32(uint32_t u) { return __uint_as_float(u); }

// Lanes of a workgroup: lx = tid & (LX - 1) walks a pair of rows, tid >> lx_log2 picks one of NT_T / LX pairs of
// rows (z, z + 1) x (y, y + 1); row pairs are dealt to the workgroups round-robin.  vector_ok: the base
// pointer and the row pitch are multiples of 16 bytes, a lane loads 16 bytes of each of the four rows (four
// cells of uint16, two of fp32) and the loads of a wave are contiguous; otherwise a lane takes one cell
// with eight element loads.
template <class T>
__global__ __launch_bounds__(NT_T) void noise_table_kernel(const T* __restrict__ vol, int nz, int ny, int nx,
                                                           int shift, int vector_ok, int lx_log2,
                                                           unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ sum_s,
                                                           unsigned long long* __restrict__ skipped) {
    extern __shared__ unsigned long long nt_lds[];
    NoiseLds L;
    L.sums = nt_lds;
    L.bins = reinterpret_cast<uint32_t*>(nt_lds + NOISE_LEVELS * NT_COLS);
    int* tags = reinterpret_cast<int*>(L.bins + NT_SLOTS * NOISE_BINS);
    L.tags = tags;
    L.skipped = reinterpret_cast<uint32_t*>(tags + NT_SLOTS);
    const int tid = threadIdx.x;
    for (int i = tid; i < NOISE_LEVELS * NT_COLS; i += NT_T) L.sums[i] = 0ull;
    for (int i = tid; i < NT_SLOTS * NOISE_BINS; i += NT_T) L.bins[i] = 0u;
    if (tid < NT_SLOTS) tags[tid] = -1;
    if (tid == NT_SLOTS) *L.skipped = 0u;
    __syncthreads();

    constexpr int VE = 16 / (int)sizeof(T);            // elements of a 16-byte vector
    const uint32_t cy = (uint32_t)ny >> 1;
    const uint32_t npr = ((uint32_t)nz >> 1) * cy;     // pairs of rows, < 2^31 (checked by the launcher)
    const int per_row = vector_ok ? nx / VE : nx >> 1; // work items of a pair of rows
    const int LX = 1 << lx_log2;
    const int lx = tid & (LX - 1);
    const uint32_t rows_per_wg = (uint32_t)(NT_T >> lx_log2);
    const size_t pitch = (size_t)nx, plane = (size_t)ny * nx;
    for (uint32_t pr = blockIdx.x * rows_per_wg + (uint32_t)(tid >> lx_log2); pr < npr;
         pr += gridDim.x * rows_per_wg) {
        const uint32_t zc = pr / cy, yc = pr - zc * cy;
        const T* row = vol + (size_t)(2 * zc) * plane + (size_t)(2 * yc) * pitch;
        for (int v = lx; v < per_row; v += LX) {
            if (vector_ok) {
                const T* p = row + (size_t)v * VE;
                const uint4 r00 = *reinterpret_cast<const uint4*>(p);
                const uint4 r01 = *reinterpret_cast<const uint4*>(p + pitch);
                const uint4 r10 = *reinterpret_cast<const uint4*>(p + plane);
                const uint4 r11 = *reinterpret_cast<const uint4*>(p + plane + pitch);
                if constexpr (sizeof(T) == 2) {
                    cell_u16(L, r00.x, r01.x, r10.x, r11.x, shift, hist);
                    cell_u16(L, r00.y, r01.y, r10.y, r11.y, shift, hist);
                    cell_u16(L, r00.z, r01.z, r10.z, r11.z, shift, hist);
                    cell_u16(L, r00.w, r01.w, r10.w, r11.w, shift, hist);
                } else {
                    cell_f32(L, as_f32(r00.x), as_f32(r00.y), as_f32(r01.x), as_f32(r01.y), as_f32(r10.x),
                             as_f32(r10.y), as_f32(r11.x), as_f32(r11.y), shift, hist);
                    cell_f32(L, as_f32(r00.z), as_f32(r00.w), as_f32(r01.z), as_f32(r01.w), as_f32(r10.z),
                             as_f32(r10.w), as_f32(r11.z), as_f32(r11.w), shift, hist);
                }
            } else {
                const T* p = row + 2 * (size_t)v;
                if constexpr (sizeof(T) == 2) {
                    cell_u16(L, (uint32_t)p[0] | ((uint32_t)p[1] << 16),
                             (uint32_t)p[pitch] | ((uint32_t)p[pitch + 1] << 16),
                             (uint32_t)p[plane] | ((uint32_t)p[plane + 1] << 16),
                             (uint32_t)p[plane + pitch] | ((uint32_t)p[plane + pitch + 1] << 16), shift, hist);
                } else {
                    cell_f32(L, p[0], p[1], p[pitch], p[pitch + 1], p[plane], p[plane + 1], p[plane + pitch],
                             p[plane + pitch + 1], shift, hist);
                }
            }
        }
    }
    __syncthreads();

    for (int slot = 0; slot < NT_SLOTS; slot++) {
        const int tag = tags[slot];
        if (tag < 0) continue;
        for (int i = tid; i < NOISE_BINS; i += NT_T) {
            const uint32_t c = L.bins[slot * NOISE_BINS + i];
            if (c) atomicAdd(&hist[(size_t)tag * NOISE_BINS + i], (unsigned long long)c);
        }
    }
    if (tid < NOISE_LEVELS) {
        unsigned long long t = 0ull;
        for (int c = 0; c < NT_COLS; c++) t += L.sums[tid * NT_COLS + c];
        if (t) atomicAdd(&sum_s[tid], t);
    }
    if (tid == NOISE_LEVELS && *L.skipped) atomicAdd(skipped, (unsigned long long)*L.skipped);
}

template <class T>
static hipError_t launch_noise_t(const T* vol, int nz, int ny, int nx, int shift, int wgs, unsigned long long* table,
                                 hipStream_t s) {
    hipError_t e = hipMemsetAsync(table, 0, noise_table_bytes(), s);
    if (e != hipSuccess) return e;
    constexpr int VE = 16 / (int)sizeof(T);
    const bool vector_ok = ((uintptr_t)vol & 15u) == 0 && ((size_t)nx * sizeof(T)) % 16 == 0;
    const int per_row = vector_ok ? nx / VE : nx / 2;
    int lx_log2 = 0;
    while ((1 << lx_log2) < per_row && (1 << lx_log2) < NT_T) lx_log2++;
    const unsigned rows_per_wg = (unsigned)(NT_T >> lx_log2);
    const unsigned npr = (unsigned)(nz / 2) * (unsigned)(ny / 2);
    unsigned blocks = (npr + rows_per_wg - 1) / rows_per_wg;
    // 140.3 KB (of 1024 B) of LDS: one workgroup per CU, and every workgroup flushes its rows once
    const unsigned resident = wgs > 0 ? (unsigned)wgs : 1u;
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL(noise_table_kernel<T>, dim3(blocks), dim3(NT_T), NT_LDS, s, vol, nz, ny, nx, shift,
                       vector_ok ? 1 : 0, lx_log2, table, table + (size_t)NOISE_LEVELS * NOISE_BINS,
                       table + (size_t)NOISE_LEVELS * NOISE_BINS + NOISE_LEVELS);
    return hipGetLastError();
}

size_t noise_table_bytes() { return ((size_t)NOISE_LEVELS * NOISE_BINS + NOISE_LEVELS + 1) * sizeof(unsigned long long); }

hipError_t noise_table_prepare(int device, int* wgs) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&noise_table_kernel<uint16_t>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)NT_LDS);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&noise_table_kernel<float>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)NT_LDS);
    if (e != hipSuccess) return e;
    int cus = 0;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return e;
    *wgs = cus > 0 ? cus : 1;
    return hipSuccess;
}

hipError_t launch_noise_table(const void* vol, int dtype, int nz, int ny, int nx, int shift, int wgs,
                              unsigned long long* table, hipStream_t s) {
    if (dtype == 0) return launch_noise_t(static_cast<const uint16_t*>(vol), nz, ny, nx, shift, wgs, table, s);
    return launch_noise_t(static_cast<const float*>(vol), nz, ny, nx, shift, wgs, table, s);
}

}  // namespace exabm4d
