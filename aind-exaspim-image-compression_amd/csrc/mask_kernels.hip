// mask_kernels.hip -- SURVEY.md section 8 row f-4: the patch-cache mask builders and
// the coherence gate of the reference's machine_learning/metrics.py:32-303, on batches of patches
// (B, nz, ny, nx) that live in HBM (gfx950).
//
//   fg_threshold_kernel   per-patch median and MAD by an exact radix selection on order-preserving
//                         fp32 keys, then thr = med + k * (1.4826 * mad), every step in fp32 like
//                         make_foreground_mask (metrics.py:55-59); NaN wherever numpy's medians are
//                         NaN (a NaN voxel, an infinite median).  One workgroup per patch.
//   dilate_kernel         one iteration of scipy.ndimage.binary_dilation with the 6-neighbour cross
//                         and border_value 0; the first iteration can read raw > thr[b] instead of
//                         a mask (the threshold fused into the first pass), or labels > 0.
//   gauss1d_kernel        one axis of scipy.ndimage.gaussian_filter in fp64 with scipy's "reflect"
//                         boundary (period 2n, so axes shorter than the radius reflect again) and
//                         scipy's symmetric accumulation order (ni_filters.c NI_Correlate1D).
//   label_set_kernel      the distinct positive labels of each patch and their voxel counts: an
//                         open-addressing hash set in LDS, one workgroup per patch; a patch with more
//                         than LS_MAX distinct labels reports status 1 and the host finishes it.
//   segment_stats_kernel  one workgroup per (patch, label): two passes, the second centred on the
//                         means of the first -- lagged pair means and Sxx / Syy / Sxy per axis, and
//                         the mean / centred sum of squares of raw and raw - smooth over the segment.
//
// Every floating-point result is deterministic: fixed thread-to-voxel mappings and fixed-order
// workgroup reductions, no floating-point atomics (the LDS atomics are integer counters).
#include "exabm4d_kernels.h"
#include "mask_src.h"

namespace exabm4d {

// ---- per-patch threshold: exact median / MAD by radix selection ------------------------------------
constexpr int SEL_T = 1024;
constexpr int SEL_W = SEL_T / 64;
constexpr uint32_t SEL_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t f32_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <class T>
struct RawVal {
    const T* p;
    __device__ float operator()(size_t i) const { return (float)p[i]; }
};
template <class T>
struct AbsDev {
    const T* p;
    float c;
    __device__ float operator()(size_t i) const { return fabsf((float)p[i] - c); }
};

// The keys of ranks r[0] and r[1] (0-based, ascending) of f(0 .. n-1): four passes of 8-bit digits,
// both ranks at once.  hist: SEL_W per-wave sub-histograms of 2 x 256 counters, then 2 x 256 totals.
// Returns whether some f(i) is NaN (the same for every thread): a NaN has a key like any other value and
// would be ranked as an extreme, where numpy's median of such data is NaN.
template <class F>
__device__ bool radix_select2(F f, size_t n, const uint32_t (&rank)[2], uint32_t* hist,
                              uint32_t* state /* [4]: prefix 0, 1, remaining rank 0, 1 */,
                              uint32_t (&key)[2]) {
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    bool nan = false;
    if (tid == 0) {
        state[0] = state[1] = 0u;
        state[2] = rank[0];
        state[3] = rank[1];
    }
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < SEL_W * 512; i += SEL_T) hist[i] = 0u;
        __syncthreads();
        const uint32_t pre0 = state[0], pre1 = state[1];
        uint32_t* h = hist + wave * 512;
        for (size_t base = 0; base < n; base += SEL_T) {
            const size_t i = base + tid;
            uint32_t b0 = SEL_NONE, b1 = SEL_NONE;
            if (i < n) {
                const float v = f(i);
                if (pass == 0) nan |= v != v;
                const uint32_t k = f32_key(v);
                const uint32_t hi = pass == 0 ? 0u : (k >> (shift + 8));
                const uint32_t d = (k >> shift) & 255u;
                if (hi == pre0) b0 = d;
                if (hi == pre1) b1 = 256u + d;
            }
            // most lanes of a wave often share a bin: one add of 64 instead of 64 serialised adds
            const uint32_t f0 = __shfl(b0, 0), f1 = __shfl(b1, 0);
            if (__all(b0 == f0)) {
                if (lane == 0 && f0 != SEL_NONE) atomicAdd(&h[f0], 64u);
            } else if (b0 != SEL_NONE) {
                atomicAdd(&h[b0], 1u);
            }
            if (__all(b1 == f1)) {
                if (lane == 0 && f1 != SEL_NONE) atomicAdd(&h[f1], 64u);
            } else if (b1 != SEL_NONE) {
                atomicAdd(&h[b1], 1u);
            }
        }
        __syncthreads();
        uint32_t* tot = hist + SEL_W * 512;
        for (int b = tid; b < 512; b += SEL_T) {
            uint32_t s = 0;
            for (int w = 0; w < SEL_W; w++) s += hist[w * 512 + b];
            tot[b] = s;
        }
        __syncthreads();
        if (tid < 2) {
            uint32_t r = state[2 + tid], c = 0;
            int d = 0;
            for (; d < 255; d++) {
                const uint32_t t = tot[tid * 256 + d];
                if (r < c + t) break;
                c += t;
            }
            state[2 + tid] = r - c;
            state[tid] = (state[tid] << 8) | (uint32_t)d;
        }
        __syncthreads();
    }
    key[0] = state[0];
    key[1] = state[1];
    return __syncthreads_or(nan) != 0;
}

// numpy's median of float32 data: the middle value, or the float32 mean of the two middle values
__device__ __forceinline__ float median_of(const uint32_t (&key)[2], bool even) {
    const float a = key_f32(key[0]), b = key_f32(key[1]);
    return even ? (a + b) / 2.0f : a;
}

template <class T>
__global__ __launch_bounds__(SEL_T) void fg_threshold_kernel(const T* __restrict__ raw, size_t n, float k,
                                                             float* __restrict__ thr) {
    __shared__ uint32_t hist[SEL_W * 512 + 512];
    __shared__ uint32_t state[4];
    const T* p = raw + (size_t)blockIdx.x * n;
    const bool even = (n % 2) == 0;
    const uint32_t rank[2] = {(uint32_t)(even ? n / 2 - 1 : n / 2), (uint32_t)(n / 2)};
    uint32_t key[2];
    bool nan = radix_select2(RawVal<T>{p}, n, rank, hist, state, key);
    const float med = median_of(key, even);
    // an infinite median makes |raw - med| NaN where raw equals it, as in numpy: caught here as well
    nan |= radix_select2(AbsDev<T>{p, med}, n, rank, hist, state, key);
    const float mad = median_of(key, even) + (float)1e-6;   // numpy rounds the Python floats to fp32
    const float sigma = (float)1.4826 * mad;
    const float ks = k * sigma;
    if (threadIdx.x == 0) thr[blockIdx.x] = nan ? __uint_as_float(0x7FC00000u) : med + ks;
}

hipError_t launch_fg_threshold(const void* raw, int dtype, int batch, size_t n, float k, float* thr,
                               hipStream_t s) {
    if (dtype == 0)
        hipLaunchKernelGGL(fg_threshold_kernel<uint16_t>, dim3(batch), dim3(SEL_T), 0, s,
                           (const uint16_t*)raw, n, k, thr);
    else
        hipLaunchKernelGGL(fg_threshold_kernel<float>, dim3(batch), dim3(SEL_T), 0, s, (const float*)raw,
                           n, k, thr);
    return hipGetLastError();
}

// ---- binary dilation, 6-neighbour cross, border_value 0 ---------------------------------------------
constexpr int DIL_T = 256;

// the sources (AboveThr, MaskSrc, LabelSrc) are in mask_src.h

// out[v] = src(v) or src of a face neighbour inside the patch; iterate == 0 only copies src
template <class Src>
__global__ __launch_bounds__(DIL_T) void dilate_kernel(Src src, int nz, int ny, int nx, size_t total,
                                                       int iterate, uint8_t* __restrict__ out) {
    const size_t plane = (size_t)ny * nx, n = plane * nz;
    for (size_t i = (size_t)blockIdx.x * DIL_T + threadIdx.x; i < total; i += (size_t)gridDim.x * DIL_T) {
        bool m = src(i);
        if (iterate && !m) {
            const size_t v = i % n;
            const int x = (int)(v % nx), y = (int)((v / nx) % ny), z = (int)(v / plane);
            m = (x > 0 && src(i - 1)) || (x + 1 < nx && src(i + 1)) ||
                (y > 0 && src(i - nx)) || (y + 1 < ny && src(i + nx)) ||
                (z > 0 && src(i - plane)) || (z + 1 < nz && src(i + plane));
        }
        out[i] = m ? 1 : 0;
    }
}

static unsigned grid_for(size_t total, int threads) {
    size_t b = (total + threads - 1) / threads;
    if (b > 65536) b = 65536;
    return (unsigned)(b ? b : 1);
}

// `iterations` passes of the cross ping-ponging between out and tmp, arranged so that the last one writes out;
// first(grid, iterate, dst) launches pass 0 from the caller's source, the later passes read the mask before them.
template <class First>
static hipError_t dilate_passes(First&& first, int batch, int nz, int ny, int nx, int iterations, uint8_t* tmp,
                                uint8_t* out, hipStream_t s) {
    const size_t n = (size_t)nz * ny * nx, total = n * batch;
    const unsigned g = grid_for(total, DIL_T);
    const int passes = iterations > 0 ? iterations : 1;
    const int iterate = iterations > 0 ? 1 : 0;
    for (int it = 0; it < passes; it++) {
        uint8_t* dst = ((passes - 1 - it) % 2 == 0) ? out : tmp;
        if (it == 0) {
            first(g, iterate, dst);
        } else {
            const uint8_t* srcp = ((passes - it) % 2 == 0) ? out : tmp;
            hipLaunchKernelGGL(dilate_kernel<MaskSrc>, dim3(g), dim3(DIL_T), 0, s, MaskSrc{srcp}, nz, ny, nx,
                               total, iterate, dst);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <class Src>
static void dilate_from(Src src, unsigned g, int nz, int ny, int nx, size_t total, int iterate, uint8_t* dst,
                        hipStream_t s) {
    hipLaunchKernelGGL(dilate_kernel<Src>, dim3(g), dim3(DIL_T), 0, s, src, nz, ny, nx, total, iterate, dst);
}

// iterations of the cross on a batch of masks (or of raw > thr when thr != NULL)
hipError_t launch_dilate(const uint8_t* in, const void* raw, int raw_dtype, const float* thr, int batch,
                         int nz, int ny, int nx, int iterations, uint8_t* tmp, uint8_t* out,
                         hipStream_t s) {
    const size_t n = (size_t)nz * ny * nx, total = n * batch;
    return dilate_passes(
        [&](unsigned g, int iterate, uint8_t* dst) {
            if (thr && raw_dtype == 0)
                dilate_from(AboveThr<uint16_t>{(const uint16_t*)raw, thr, n}, g, nz, ny, nx, total, iterate, dst, s);
            else if (thr)
                dilate_from(AboveThr<float>{(const float*)raw, thr, n}, g, nz, ny, nx, total, iterate, dst, s);
            else
                dilate_from(MaskSrc{in}, g, nz, ny, nx, total, iterate, dst, s);
        },
        batch, nz, ny, nx, iterations, tmp, out, s);
}

// the same on labels > 0 (make_segmentation_mask): the comparison is fused into the first pass
hipError_t launch_dilate_labels(const void* labels, int ldtype, int batch, int nz, int ny, int nx, int iterations,
                                uint8_t* tmp, uint8_t* out, hipStream_t s) {
    const size_t total = (size_t)nz * ny * nx * batch;
    return dilate_passes(
        [&](unsigned g, int iterate, uint8_t* dst) {
            switch (ldtype) {
                case LBL_U8: dilate_from(LabelSrc<uint8_t>{(const uint8_t*)labels}, g, nz, ny, nx, total, iterate, dst, s); break;
                case LBL_U32: dilate_from(LabelSrc<uint32_t>{(const uint32_t*)labels}, g, nz, ny, nx, total, iterate, dst, s); break;
                case LBL_U64: dilate_from(LabelSrc<uint64_t>{(const uint64_t*)labels}, g, nz, ny, nx, total, iterate, dst, s); break;
                case LBL_I32: dilate_from(LabelSrc<int32_t>{(const int32_t*)labels}, g, nz, ny, nx, total, iterate, dst, s); break;
                default: dilate_from(LabelSrc<int64_t>{(const int64_t*)labels}, g, nz, ny, nx, total, iterate, dst, s); break;
            }
        },
        batch, nz, ny, nx, iterations, tmp, out, s);
}

// ---- Gaussian smoothing, one axis, fp64 ---------------------------------------------------------------
constexpr int GF_T = 256;

__device__ __forceinline__ int reflect_2n(int i, int len) {
    const int p = 2 * len;
    int m = i % p;
    if (m < 0) m += p;
    return m < len ? m : p - 1 - m;
}

template <class T>
__global__ __launch_bounds__(GF_T) void gauss1d_kernel(const T* __restrict__ src, double* __restrict__ dst,
                                                       int nz, int ny, int nx, size_t total, int axis,
                                                       GaussWeights w) {
    const size_t plane = (size_t)ny * nx, n = plane * nz;
    const int len = axis == 0 ? nz : (axis == 1 ? ny : nx);
    const size_t stride = axis == 0 ? plane : (axis == 1 ? (size_t)nx : 1);
    for (size_t i = (size_t)blockIdx.x * GF_T + threadIdx.x; i < total; i += (size_t)gridDim.x * GF_T) {
        const size_t v = i % n;
        const int c = axis == 0 ? (int)(v / plane) : (axis == 1 ? (int)((v / nx) % ny) : (int)(v % nx));
        const size_t line = i - (size_t)c * stride;
        double acc = (double)src[i] * w.w[0];
        for (int j = w.radius; j >= 1; j--) {
            const double lo = (double)src[line + (size_t)reflect_2n(c - j, len) * stride];
            const double hi = (double)src[line + (size_t)reflect_2n(c + j, len) * stride];
            acc += (lo + hi) * w.w[j];
        }
        dst[i] = acc;
    }
}

// axes 0, 1, 2 in that order: src -> out -> tmp -> out
hipError_t launch_gaussian3d(const void* src, int dtype, int batch, int nz, int ny, int nx,
                             const GaussWeights& w, double* tmp, double* out, hipStream_t s) {
    const size_t total = (size_t)nz * ny * nx * batch;
    const unsigned g = grid_for(total, GF_T);
    if (dtype == 1)
        hipLaunchKernelGGL(gauss1d_kernel<float>, dim3(g), dim3(GF_T), 0, s, (const float*)src, out, nz, ny, nx,
                           total, 0, w);
    else
        hipLaunchKernelGGL(gauss1d_kernel<double>, dim3(g), dim3(GF_T), 0, s, (const double*)src, out, nz, ny,
                           nx, total, 0, w);
    hipLaunchKernelGGL(gauss1d_kernel<double>, dim3(g), dim3(GF_T), 0, s, (const double*)out, tmp, nz, ny, nx,
                       total, 1, w);
    hipLaunchKernelGGL(gauss1d_kernel<double>, dim3(g), dim3(GF_T), 0, s, (const double*)tmp, out, nz, ny, nx,
                       total, 2, w);
    return hipGetLastError();
}

// ---- distinct positive labels per patch -------------------------------------------------------------
constexpr int LS_T = 1024;
constexpr int LS_SLOTS = 2 * LS_MAX;   // load factor <= 1/2

template <class T>
__device__ __forceinline__ unsigned long long label_key(T v) {
    return v > (T)0 ? (unsigned long long)v : 0ull;   // 0 = background (and the empty slot)
}

__device__ __forceinline__ uint32_t ls_hash(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (uint32_t)k & (LS_SLOTS - 1);
}

// Insert c voxels of key k.  A new key is refused once LS_MAX keys are held (the check races, so up to
// LS_T - 1 more may land: the table has 2 * LS_MAX slots and the caller flags any excess); false = refused.
// `used` is raised after a claim, so once it reads LS_MAX the slots of LS_MAX keys are visible: a slot seen
// empty before that is read again, since the thread that filled the set may have claimed it for this very key.
__device__ bool ls_insert(unsigned long long* keys, uint32_t* counts, uint32_t* used, unsigned long long k,
                          uint32_t c) {
    uint32_t h = ls_hash(k);
    for (int probe = 0; probe < LS_SLOTS; probe++, h = (h + 1) & (LS_SLOTS - 1)) {
        unsigned long long cur = *(volatile unsigned long long*)&keys[h];
        if (cur == 0ull) {
            if (*(volatile uint32_t*)used < (uint32_t)LS_MAX) {
                cur = atomicCAS(&keys[h], 0ull, k);
                if (cur == 0ull) {
                    atomicAdd(used, 1u);
                    cur = k;
                }
            } else {
                cur = *(volatile unsigned long long*)&keys[h];
                if (cur == 0ull) return false;
            }
        }
        if (cur == k) {
            atomicAdd(&counts[h], c);
            return true;
        }
    }
    return false;
}

template <class T>
__global__ __launch_bounds__(LS_T) void label_set_kernel(const T* __restrict__ labels, size_t n,
                                                         unsigned long long* __restrict__ keys_out,
                                                         uint32_t* __restrict__ counts_out,
                                                         uint32_t* __restrict__ n_out,
                                                         uint32_t* __restrict__ status) {
    __shared__ unsigned long long keys[LS_SLOTS];
    __shared__ uint32_t counts[LS_SLOTS];
    __shared__ uint32_t used, full, nout;
    const int tid = threadIdx.x, lane = tid % 64;
    for (int i = tid; i < LS_SLOTS; i += LS_T) {
        keys[i] = 0ull;
        counts[i] = 0u;
    }
    if (tid == 0) used = full = nout = 0u;
    __syncthreads();
    const T* p = labels + (size_t)blockIdx.x * n;
    for (size_t base = 0; base < n; base += LS_T) {
        if (*(volatile uint32_t*)&full) break;   // the host redoes this patch: stop early (wave-uniform read)
        const size_t i = base + tid;
        const unsigned long long k = i < n ? label_key(p[i]) : 0ull;
        const unsigned long long first = __shfl(k, 0);
        if (__all(k == first)) {
            if (lane == 0 && k != 0ull && !ls_insert(keys, counts, &used, k, 64u)) full = 1u;
        } else if (k != 0ull && !ls_insert(keys, counts, &used, k, 1u)) {
            full = 1u;
        }
    }
    __syncthreads();
    unsigned long long* ko = keys_out + (size_t)blockIdx.x * LS_MAX;
    uint32_t* co = counts_out + (size_t)blockIdx.x * LS_MAX;
    for (int i = tid; i < LS_SLOTS; i += LS_T) {
        if (keys[i] != 0ull) {
            const uint32_t j = atomicAdd(&nout, 1u);   // slot order; the host sorts the keys
            if (j < (uint32_t)LS_MAX) {
                ko[j] = keys[i];
                co[j] = counts[i];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        n_out[blockIdx.x] = nout < (uint32_t)LS_MAX ? nout : (uint32_t)LS_MAX;
        status[blockIdx.x] = (full || used > (uint32_t)LS_MAX) ? 1u : 0u;
    }
}

hipError_t launch_label_set(const void* labels, int ldtype, int batch, size_t n, unsigned long long* keys,
                            uint32_t* counts, uint32_t* n_out, uint32_t* status, hipStream_t s) {
    switch (ldtype) {
        case LBL_U8: hipLaunchKernelGGL(label_set_kernel<uint8_t>, dim3(batch), dim3(LS_T), 0, s, (const uint8_t*)labels, n, keys, counts, n_out, status); break;
        case LBL_U32: hipLaunchKernelGGL(label_set_kernel<uint32_t>, dim3(batch), dim3(LS_T), 0, s, (const uint32_t*)labels, n, keys, counts, n_out, status); break;
        case LBL_U64: hipLaunchKernelGGL(label_set_kernel<uint64_t>, dim3(batch), dim3(LS_T), 0, s, (const uint64_t*)labels, n, keys, counts, n_out, status); break;
        case LBL_I32: hipLaunchKernelGGL(label_set_kernel<int32_t>, dim3(batch), dim3(LS_T), 0, s, (const int32_t*)labels, n, keys, counts, n_out, status); break;
        default: hipLaunchKernelGGL(label_set_kernel<int64_t>, dim3(batch), dim3(LS_T), 0, s, (const int64_t*)labels, n, keys, counts, n_out, status); break;
    }
    return hipGetLastError();
}

// ---- segment statistics, two passes, centred -----------------------------------------------------------
constexpr int SS_T = 256;

template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sh) {
    for (int k = 0; k < K; k++) {
        sh[threadIdx.x] = v[k];
        __syncthreads();
        for (int s = SS_T / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        v[k] = sh[0];
        __syncthreads();
    }
}

// out[item * SEG_STATS_K]: n, mean raw, mean (raw - smooth), centred SS of raw, centred SS of
// raw - smooth, then per axis: pairs, mean x, mean y, Sxx, Syy, Sxy
template <class TL, class TR>
__global__ __launch_bounds__(SS_T) void segment_stats_kernel(const TL* __restrict__ labels,
                                                             const TR* __restrict__ raw,
                                                             const double* __restrict__ smooth,
                                                             int nz, int ny, int nx, int lag,
                                                             const int32_t* __restrict__ item_patch,
                                                             const unsigned long long* __restrict__ item_key,
                                                             double* __restrict__ out) {
    __shared__ double sh[SS_T];
    const size_t plane = (size_t)ny * nx, n = plane * nz;
    const size_t off = (size_t)item_patch[blockIdx.x] * n;
    const TL* L = labels + off;
    const TR* R = raw + off;
    const double* S = smooth ? smooth + off : nullptr;
    const unsigned long long key = item_key[blockIdx.x];
    const size_t step[3] = {plane * lag, (size_t)nx * lag, (size_t)lag};
    const int lim[3] = {nz - lag, ny - lag, nx - lag};
    // pass 1: counts and sums
    double a[12] = {};
    for (size_t v = threadIdx.x; v < n; v += SS_T) {
        if (label_key(L[v]) != key) continue;
        const double r = (double)R[v];
        a[0] += 1.0;
        a[1] += r;
        if (S) a[2] += r - S[v];
        const int c[3] = {(int)(v / plane), (int)((v / nx) % ny), (int)(v % nx)};
        for (int ax = 0; ax < 3; ax++) {
            if (c[ax] >= lim[ax] || label_key(L[v + step[ax]]) != key) continue;
            a[3 + 3 * ax] += 1.0;
            a[4 + 3 * ax] += r;
            a[5 + 3 * ax] += (double)R[v + step[ax]];
        }
    }
    block_sum(a, sh);
    const double mr = a[0] > 0.0 ? a[1] / a[0] : 0.0, mh = a[0] > 0.0 ? a[2] / a[0] : 0.0;
    double mx[3], my[3];
    for (int ax = 0; ax < 3; ax++) {
        const double np = a[3 + 3 * ax];
        mx[ax] = np > 0.0 ? a[4 + 3 * ax] / np : 0.0;
        my[ax] = np > 0.0 ? a[5 + 3 * ax] / np : 0.0;
    }
    // pass 2: centred sums
    double b[11] = {};
    for (size_t v = threadIdx.x; v < n; v += SS_T) {
        if (label_key(L[v]) != key) continue;
        const double r = (double)R[v];
        const double dr = r - mr;
        b[0] += dr * dr;
        if (S) {
            const double dh = (r - S[v]) - mh;
            b[1] += dh * dh;
        }
        const int c[3] = {(int)(v / plane), (int)((v / nx) % ny), (int)(v % nx)};
        for (int ax = 0; ax < 3; ax++) {
            if (c[ax] >= lim[ax] || label_key(L[v + step[ax]]) != key) continue;
            const double dx = r - mx[ax], dy = (double)R[v + step[ax]] - my[ax];
            b[2 + 3 * ax] += dx * dx;
            b[3 + 3 * ax] += dy * dy;
            b[4 + 3 * ax] += dx * dy;
        }
    }
    block_sum(b, sh);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)blockIdx.x * SEG_STATS_K;
        o[0] = a[0];
        o[1] = mr;
        o[2] = mh;
        o[3] = b[0];
        o[4] = b[1];
        for (int ax = 0; ax < 3; ax++) {
            double* q = o + 5 + 6 * ax;
            q[0] = a[3 + 3 * ax];
            q[1] = mx[ax];
            q[2] = my[ax];
            q[3] = b[2 + 3 * ax];
            q[4] = b[3 + 3 * ax];
            q[5] = b[4 + 3 * ax];
        }
    }
}

template <class TL>
static void launch_ss_l(const TL* labels, const void* raw, int rdtype, const double* smooth, int nz, int ny,
                        int nx, int lag, const int32_t* ip, const unsigned long long* ik, int items,
                        double* out, hipStream_t s) {
    if (rdtype == 1)
        hipLaunchKernelGGL((segment_stats_kernel<TL, float>), dim3(items), dim3(SS_T), 0, s, labels,
                           (const float*)raw, smooth, nz, ny, nx, lag, ip, ik, out);
    else
        hipLaunchKernelGGL((segment_stats_kernel<TL, double>), dim3(items), dim3(SS_T), 0, s, labels,
                           (const double*)raw, smooth, nz, ny, nx, lag, ip, ik, out);
}

hipError_t launch_segment_stats(const void* labels, int ldtype, const void* raw, int rdtype, const double* smooth,
                                int nz, int ny, int nx, int lag, const int32_t* item_patch,
                                const unsigned long long* item_key, int items, double* out, hipStream_t s) {
    switch (ldtype) {
        case LBL_U8: launch_ss_l((const uint8_t*)labels, raw, rdtype, smooth, nz, ny, nx, lag, item_patch, item_key, items, out, s); break;
        case LBL_U32: launch_ss_l((const uint32_t*)labels, raw, rdtype, smooth, nz, ny, nx, lag, item_patch, item_key, items, out, s); break;
        case LBL_U64: launch_ss_l((const uint64_t*)labels, raw, rdtype, smooth, nz, ny, nx, lag, item_patch, item_key, items, out, s); break;
        case LBL_I32: launch_ss_l((const int32_t*)labels, raw, rdtype, smooth, nz, ny, nx, lag, item_patch, item_key, items, out, s); break;
        default: launch_ss_l((const int64_t*)labels, raw, rdtype, smooth, nz, ny, nx, lag, item_patch, item_key, items, out, s); break;
    }
    return hipGetLastError();
}

}  // namespace exabm4d
