// validate_kernels.hip -- DESIGN.md 5.12: the count-space metrics of a validation batch (the reference's
// machine_learning/metrics.py:352-424 under Trainer.validate), one row of VAL_K doubles per patch of a
// (B, n) batch that lives in HBM (gfx950).
//
//   validate_select_kernel  two workgroups per patch.  Job 0: the raw values at the two median ranks and the two
//                           percentile ranks by ONE exact radix selection on raw's native key (16 bits for uint16,
//                           32 for float32), med in fp64, then the two median ranks of |raw - med| on 64-bit keys of
//                           the fp64 deviations, then thr.  Job 1: the pred values at the percentile ranks.
//   validate_stats_kernel   up to VAL_MAX_SPLITS workgroups per patch: masked sums of |pred - raw| and
//                           |pred - target|, the foreground and bright-background counts (pred > thr, thr read
//                           from the row), maxima and NaN counts.
//   validate_finish_kernel  the splits' partials into the row, in split order.
//
// Every value is widened to fp64 before any arithmetic, as the reference does.  Results are deterministic and do
// not depend on the batch size: fixed thread-to-voxel mappings, a split count that depends on n alone, fixed-order
// reductions; the only atomics are integer LDS counters.
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int VS_T = 1024;          // threads of a selection workgroup
constexpr int VS_SUB = 8;           // LDS sub-histograms (wave w counts into w % VS_SUB)
constexpr int VS_R = 4;             // most ranks one selection follows
constexpr uint32_t VS_NONE = 0xFFFFFFFFu;
constexpr int VT_T = 256;           // threads of a statistics workgroup
constexpr int VT_K = 9;             // partial columns: row columns 0..5, then NaN counts of pred, raw, target
constexpr size_t VT_SPLIT = 4096;   // voxels per split, until VAL_MAX_SPLITS splits are reached

__device__ __forceinline__ double val_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
// np.max: a NaN on either side gives NaN
__device__ __forceinline__ double val_max_nan(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

// ---- order-preserving keys ----------------------------------------------------------------------------------
template <class T>
struct NativeKey;
template <>
struct NativeKey<uint16_t> {
    static constexpr int BITS = 16;
    const uint16_t* p;
    __device__ unsigned long long operator()(size_t i, bool&) const { return p[i]; }
    static __device__ double value(unsigned long long k) { return (double)k; }
};
template <>
struct NativeKey<float> {
    static constexpr int BITS = 32;
    const float* p;
    __device__ unsigned long long operator()(size_t i, bool& nan) const {
        const float v = p[i];
        nan |= v != v;
        const uint32_t b = __float_as_uint(v);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    static __device__ double value(unsigned long long k) {
        const uint32_t b = (uint32_t)k;
        return (double)__uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
    }
};
// |p[i] - c| in fp64: differences of neighbouring float32 values are not float32 values
template <class T>
struct DevKey {
    static constexpr int BITS = 64;
    const T* p;
    double c;
    __device__ unsigned long long operator()(size_t i, bool& nan) const {
        const double v = fabs((double)p[i] - c);
        nan |= v != v;
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    static __device__ double value(unsigned long long k) {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
    }
};

struct SelState {
    unsigned long long prefix[VS_R];    // the digits chosen so far
    uint32_t rem[VS_R];                 // rank among the elements that share the prefix
    int alias[VS_R];                    // the first rank with the same prefix: its histogram serves both
};

// The keys of ranks rank[0 .. R-1] (0-based) of f(0 .. n-1), 8 bits per pass from the top.  Ranks whose prefixes
// agree share one histogram, so neighbouring ranks cost one count per voxel until their digits part.
// hist: VS_SUB sub-histograms of R x 256 counters, then R x 256 totals.  Returns whether some f(i) is NaN (the same
// for every thread): a NaN has a key like any other value and would be ranked as an extreme.
template <int R, class F>
__device__ bool select_ranks(F f, size_t n, const uint32_t (&rank)[R], uint32_t* hist, SelState* st,
                             unsigned long long (&key)[R]) {
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    bool nan = false;
    if (tid == 0)
        for (int r = 0; r < R; r++) {
            st->prefix[r] = 0ull;
            st->rem[r] = rank[r];
            st->alias[r] = 0;
        }
    for (int pass = 0; pass < F::BITS / 8; pass++) {
        const int shift = F::BITS - 8 * (pass + 1);
        for (int i = tid; i < VS_SUB * R * 256; i += VS_T) hist[i] = 0u;
        __syncthreads();
        unsigned long long pre[R];
        bool own[R];
        for (int r = 0; r < R; r++) {
            pre[r] = st->prefix[r];
            own[r] = st->alias[r] == r;
        }
        uint32_t* h = hist + (wave % VS_SUB) * (R * 256);
        for (size_t base = 0; base < n; base += VS_T) {
            const size_t i = base + tid;
            uint32_t b[R];
            for (int r = 0; r < R; r++) b[r] = VS_NONE;
            if (i < n) {
                const unsigned long long k = f(i, nan);
                const unsigned long long hi = pass == 0 ? 0ull : (k >> (shift + 8));
                const uint32_t d = (uint32_t)(k >> shift) & 255u;
                for (int r = 0; r < R; r++)
                    if (own[r] && hi == pre[r]) b[r] = (uint32_t)r * 256u + d;
            }
            for (int r = 0; r < R; r++) {
                if (!own[r]) continue;          // the same for every thread of the workgroup
                // most lanes of a wave often share a bin: one add of 64 instead of 64 serialised adds
                const uint32_t f0 = __shfl(b[r], 0);
                if (__all(b[r] == f0)) {
                    if (lane == 0 && f0 != VS_NONE) atomicAdd(&h[f0], 64u);
                } else if (b[r] != VS_NONE) {
                    atomicAdd(&h[b[r]], 1u);
                }
            }
        }
        __syncthreads();
        uint32_t* tot = hist + VS_SUB * R * 256;
        for (int bin = tid; bin < R * 256; bin += VS_T) {
            uint32_t s = 0;
            for (int w = 0; w < VS_SUB; w++) s += hist[w * (R * 256) + bin];
            tot[bin] = s;
        }
        __syncthreads();
        if (tid < R) {
            const uint32_t* t = tot + st->alias[tid] * 256;
            uint32_t r = st->rem[tid], c = 0;
            int d = 0;
            for (; d < 255; d++) {
                if (r < c + t[d]) break;
                c += t[d];
            }
            st->rem[tid] = r - c;
            st->prefix[tid] = (st->prefix[tid] << 8) | (unsigned long long)d;
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < R; r++) {
                int a = r;
                for (int q = r - 1; q >= 0; q--)
                    if (st->prefix[q] == st->prefix[r]) a = q;
                st->alias[r] = a;
            }
        __syncthreads();
    }
    for (int r = 0; r < R; r++) key[r] = st->prefix[r];
    return __syncthreads_or(nan) != 0;
}

// np.median of fp64 data: the middle value, or the mean of the two middle values
__device__ __forceinline__ double val_median(double a, double b, bool two) { return two ? (a + b) / 2.0 : a; }

template <class TP, class TR>
__global__ __launch_bounds__(VS_T) void validate_select_kernel(const TP* __restrict__ pred,
                                                               const TR* __restrict__ raw, size_t n, double k,
                                                               ValRanks rk, double* __restrict__ rows) {
    __shared__ uint32_t hist[VS_SUB * VS_R * 256 + VS_R * 256];
    __shared__ SelState st;
    const size_t patch = blockIdx.x >> 1;
    double* row = rows + patch * VAL_K;
    if ((blockIdx.x & 1u) == 0) {
        const TR* p = raw + patch * n;
        const uint32_t r4[4] = {rk.r[0], rk.r[1], rk.r[2], rk.r[3]};
        unsigned long long key[4];
        bool nan = select_ranks<4>(NativeKey<TR>{p}, n, r4, hist, &st, key);
        const bool two = rk.r[0] != rk.r[1];
        const double med = nan ? val_nan()
                               : val_median(NativeKey<TR>::value(key[0]), NativeKey<TR>::value(key[1]), two);
        const double lo = nan ? val_nan() : NativeKey<TR>::value(key[2]);
        const double hi = nan ? val_nan() : NativeKey<TR>::value(key[3]);
        // an infinite median makes |raw - med| NaN where raw equals it, as in numpy: caught here as well
        const uint32_t r2[2] = {rk.r[0], rk.r[1]};
        unsigned long long dkey[2];
        nan |= select_ranks<2>(DevKey<TR>{p, med}, n, r2, hist, &st, dkey);
        const double mad = nan ? val_nan() : val_median(DevKey<TR>::value(dkey[0]), DevKey<TR>::value(dkey[1]), two);
        // thr = med + (k * 1.4826) * (mad + 1e-6): metrics.py:379-380, each operation rounded on its own
        const double thr = __dadd_rn(med, __dmul_rn(__dmul_rn(k, 1.4826), __dadd_rn(mad, 1e-6)));
        if (threadIdx.x == 0) {
            row[VAL_MED] = med;
            row[VAL_MAD] = mad;
            row[VAL_THR] = thr;
            row[VAL_RAW_LO] = lo;
            row[VAL_RAW_HI] = hi;
        }
    } else {
        const uint32_t r2[2] = {rk.r[2], rk.r[3]};
        unsigned long long key[2];
        const bool nan = select_ranks<2>(NativeKey<TP>{pred + patch * n}, n, r2, hist, &st, key);
        if (threadIdx.x == 0) {
            row[VAL_PRED_LO] = nan ? val_nan() : NativeKey<TP>::value(key[0]);
            row[VAL_PRED_HI] = nan ? val_nan() : NativeKey<TP>::value(key[1]);
        }
    }
}

int validate_splits(size_t n) {
    const size_t s = (n + VT_SPLIT - 1) / VT_SPLIT;
    return (int)(s < 1 ? 1 : (s > (size_t)VAL_MAX_SPLITS ? (size_t)VAL_MAX_SPLITS : s));
}

// split s of a patch covers voxels [s * per, min(n, (s + 1) * per)), per = ceil(n / splits)
template <class TP, class TR, class TT>
__global__ __launch_bounds__(VT_T) void validate_stats_kernel(const TP* __restrict__ pred, const TR* __restrict__ raw,
                                                              const TT* __restrict__ target,
                                                              const uint8_t* __restrict__ mask, size_t n, int splits,
                                                              const double* __restrict__ rows,
                                                              double* __restrict__ partials) {
    __shared__ double sh[VT_T];
    const size_t patch = blockIdx.x / (unsigned)splits, split = blockIdx.x % (unsigned)splits;
    const size_t per = (n + splits - 1) / splits;
    const size_t begin = split * per, end = begin + per < n ? begin + per : n;
    const size_t off = patch * n;
    const double thr = rows[patch * VAL_K + VAL_THR];
    double v[VT_K] = {0.0, 0.0, 0.0, 0.0, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (size_t i = begin + threadIdx.x; i < end; i += VT_T) {
        const double p = (double)pred[off + i], r = (double)raw[off + i], t = (double)target[off + i];
        if (mask[off + i] != 0) {
            v[0] += fabs(p - r);
            v[2] += 1.0;
        } else {
            v[1] += fabs(p - t);
            if (p > thr) v[3] += 1.0;
        }
        v[4] = val_max_nan(v[4], p);
        v[5] = val_max_nan(v[5], r);
        if (p != p) v[6] += 1.0;
        if (r != r) v[7] += 1.0;
        if (t != t) v[8] += 1.0;
    }
    for (int c = 0; c < VT_K; c++) {
        const bool is_max = c == 4 || c == 5;
        sh[threadIdx.x] = v[c];
        __syncthreads();
        for (int s = VT_T / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                const double x = sh[threadIdx.x], y = sh[threadIdx.x + s];
                sh[threadIdx.x] = is_max ? val_max_nan(x, y) : x + y;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * VT_K + c] = sh[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void validate_finish_kernel(const double* __restrict__ partials, int splits,
                                                             double* __restrict__ rows) {
    const int c = threadIdx.x;
    if (c >= VT_K) return;
    const double* p = partials + (size_t)blockIdx.x * splits * VT_K;
    const bool is_max = c == 4 || c == 5;
    double a = is_max ? -INFINITY : 0.0;
    for (int s = 0; s < splits; s++) {
        const double x = p[(size_t)s * VT_K + c];
        a = is_max ? val_max_nan(a, x) : a + x;
    }
    double* row = rows + (size_t)blockIdx.x * VAL_K;
    if (c < 6)
        row[c] = a;
    else
        row[VAL_PRED_NAN + (c - 6)] = a > 0.0 ? 1.0 : 0.0;
}

size_t validate_partials_bytes(int batch, size_t n) {
    return (size_t)batch * validate_splits(n) * VT_K * sizeof(double);
}

template <class TP, class TR>
static hipError_t validate_launch(const TP* pred, const TR* raw, const void* target, int target_dtype,
                                  const uint8_t* mask, int batch, size_t n, double k, const ValRanks& rk,
                                  double* partials, double* rows, hipStream_t s) {
    hipLaunchKernelGGL((validate_select_kernel<TP, TR>), dim3(2u * batch), dim3(VS_T), 0, s, pred, raw, n, k, rk,
                       rows);
    const int splits = validate_splits(n);
    const dim3 grid((unsigned)batch * splits);
    if (target_dtype == 0)
        hipLaunchKernelGGL((validate_stats_kernel<TP, TR, uint16_t>), grid, dim3(VT_T), 0, s, pred, raw,
                           (const uint16_t*)target, mask, n, splits, rows, partials);
    else
        hipLaunchKernelGGL((validate_stats_kernel<TP, TR, float>), grid, dim3(VT_T), 0, s, pred, raw,
                           (const float*)target, mask, n, splits, rows, partials);
    hipLaunchKernelGGL(validate_finish_kernel, dim3(batch), dim3(64), 0, s, partials, splits, rows);
    return hipGetLastError();
}

hipError_t launch_validate_batch(const void* pred, int pred_dtype, const void* raw, int raw_dtype,
                                 const void* target, int target_dtype, const uint8_t* mask, int batch, size_t n,
                                 double k, const ValRanks& rk, double* partials, double* rows, hipStream_t s) {
    if (pred_dtype == 0) {
        if (raw_dtype == 0)
            return validate_launch((const uint16_t*)pred, (const uint16_t*)raw, target, target_dtype, mask, batch, n,
                                   k, rk, partials, rows, s);
        return validate_launch((const uint16_t*)pred, (const float*)raw, target, target_dtype, mask, batch, n, k, rk,
                               partials, rows, s);
    }
    if (raw_dtype == 0)
        return validate_launch((const float*)pred, (const uint16_t*)raw, target, target_dtype, mask, batch, n, k, rk,
                               partials, rows, s);
    return validate_launch((const float*)pred, (const float*)raw, target, target_dtype, mask, batch, n, k, rk,
                           partials, rows, s);
}

}  // namespace exabm4d
