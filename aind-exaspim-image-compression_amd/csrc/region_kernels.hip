// region_kernels.hip -- boxes gathered from a pool of decoded chunks, the read side of the chunk
// store, and boxes scattered into such a pool, its write side.  Copy kernels: every output element
// is written at most once, every element a box covers is read once.
#include "exabm4d_kernels.h"

namespace exabm4d {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / 64;

// One output element type: how a pool value becomes an element, and two elements one store.
struct PutU16 {
    using T = uint16_t;
    using T2 = uint32_t;
    T fill;
    __device__ T conv(uint16_t v) const { return v; }
    __device__ static T2 pack(T a, T b) { return (T2)a | ((T2)b << 16); }
};
struct PutF32 {
    using T = float;
    using T2 = float2;
    T fill;
    float offset;
    __device__ T conv(uint16_t v) const { return (float)v - offset; }       // one IEEE subtraction (read_counts)
    __device__ static T2 pack(T a, T b) { return make_float2(a, b); }
};

// `len` elements of a row segment, lanes along x.  `o` and `s` (NULL: fill) are wave-uniform, so every branch on
// their alignment is too.  Elements go out in pairs where the output address allows a store of twice the width;
// a source pair is one 4-byte load where the source address allows that, else two 2-byte loads.
template <typename P>
__device__ inline void put_segment(const P& p, typename P::T* o, const uint16_t* s, int len, int lane) {
    using T = typename P::T;
    using T2 = typename P::T2;
    const int head = (int)(((uintptr_t)o / sizeof(T)) & 1);           // o is aligned to sizeof(T)
    if (head && lane == 0) o[0] = s ? p.conv(s[0]) : p.fill;
    const int pairs = (len - head) >> 1;
    T2* o2 = reinterpret_cast<T2*>(o + head);
    if (!s) {
        const T2 f = P::pack(p.fill, p.fill);
        for (int i = lane; i < pairs; i += 64) o2[i] = f;
    } else if ((((uintptr_t)(s + head)) & 2) == 0) {
        const uint32_t* s2 = reinterpret_cast<const uint32_t*>(s + head);
        for (int i = lane; i < pairs; i += 64) {
            const uint32_t v = s2[i];
            o2[i] = P::pack(p.conv((uint16_t)(v & 0xFFFFu)), p.conv((uint16_t)(v >> 16)));
        }
    } else {
        const uint16_t* s1 = s + head;
        for (int i = lane; i < pairs; i += 64) o2[i] = P::pack(p.conv(s1[2 * i]), p.conv(s1[2 * i + 1]));
    }
    const int done = head + 2 * pairs;
    if (done < len && lane == 63) o[done] = s ? p.conv(s[done]) : p.fill;
}

// One wave per output row (box n, plane z, row y).  The wave walks the row in segments: at x it scans the box's
// source list for the first source that holds the voxel; the segment ends where that source ends, where a source
// listed before it begins (it wins there), or -- with no source -- where the next one begins.  All of that is
// wave-uniform (scalar loads and branches); only put_segment() uses the lanes.
template <typename P>
__global__ __launch_bounds__(RG_THREADS) void gather_boxes_kernel(
        const uint16_t* __restrict__ pool, const BoxSrc* __restrict__ srcs, const int32_t* __restrict__ lists,
        int per_box, const int32_t* __restrict__ starts, unsigned long long rows, int bz, int by, int bx, P p,
        typename P::T* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long stride = (unsigned long long)gridDim.x * RG_WAVES;
    for (unsigned long long r = (unsigned long long)blockIdx.x * RG_WAVES + wave; r < rows; r += stride) {
        const unsigned long long n = r / ((unsigned long long)bz * by);
        const unsigned rem = (unsigned)(r - n * ((unsigned long long)bz * by));
        const long long pz = (long long)starts[3 * n] + rem / (unsigned)by;
        const long long py = (long long)starts[3 * n + 1] + rem % (unsigned)by;
        const long long sx = starts[3 * n + 2];
        const int32_t* list = lists + n * (unsigned long long)per_box;
        typename P::T* orow = out + r * (unsigned long long)bx;
        int x = 0;
        while (x < bx) {
            const long long px = sx + x;
            int len = bx - x;
            const uint16_t* s = nullptr;
            for (int j = 0; j < per_box; j++) {
                const int k = list[j];
                if (k < 0) continue;
                const BoxSrc& b = srcs[k];
                if (pz < b.z0 || pz >= (long long)b.z0 + b.ez || py < b.y0 || py >= (long long)b.y0 + b.ey) continue;
                const long long x0 = b.x0, x1 = x0 + b.ex;
                if (px >= x0 && px < x1) {
                    if (x1 - px < len) len = (int)(x1 - px);
                    s = pool + b.base + (unsigned long long)(pz - b.z0) * b.stride_z +
                        (unsigned long long)(py - b.y0) * b.stride_y + (unsigned long long)(px - x0);
                    break;
                }
                if (x0 > px && x0 - px < len) len = (int)(x0 - px);
            }
            put_segment(p, orow + x, s, len, lane);
            x += len;
        }
    }
}

// ---- the write side: boxes scattered into the pool -------------------------------------------
// One element pairing of the scatter: source element S, pool element T, how one becomes the other.
struct CopyU16 {
    using S = uint16_t;
    using T = uint16_t;
    __device__ T conv(S v) const { return v; }
};
struct CopyU8 {
    using S = uint8_t;
    using T = uint8_t;
    __device__ T conv(S v) const { return v; }
};
struct CountsF32 {
    using S = float;
    using T = uint16_t;
    float offset;
    // one IEEE addition, np.clip, np.rint (ties to even), astype(uint16): exabm4d_normalize_u16_dev's tail.  fmaxf
    // returns its other operand for a NaN, so a NaN becomes 0.
    __device__ T conv(S v) const { return (uint16_t)rintf(fminf(fmaxf(v + offset, 0.0f), 65535.0f)); }
};

// Two neighbouring elements as one load or store of twice the width.
template <typename E>
struct alignas(2 * sizeof(E)) Two {
    E a, b;
};

// `len` elements of a row segment, lanes along x; `o` and `s` are wave-uniform, so every branch on their alignment
// is too.  Elements go out in pairs where the pool address allows a store of twice the width; a source pair is
// one load of twice the width where the source address allows that, else two loads.  Every element of
// [o, o + len) is written by exactly one lane and nothing else is.
template <typename C>
__device__ inline void copy_segment(const C& c, typename C::T* o, const typename C::S* s, int len, int lane) {
    using S = typename C::S;
    using T = typename C::T;
    const int head = (int)(((uintptr_t)o / sizeof(T)) & 1);           // o is aligned to sizeof(T)
    if (head && lane == 0) o[0] = c.conv(s[0]);
    const int pairs = (len - head) >> 1;
    Two<T>* o2 = reinterpret_cast<Two<T>*>(o + head);
    const S* s1 = s + head;
    if ((((uintptr_t)s1 / sizeof(S)) & 1) == 0) {
        const Two<S>* s2 = reinterpret_cast<const Two<S>*>(s1);
        for (int i = lane; i < pairs; i += 64) {
            const Two<S> v = s2[i];
            o2[i] = Two<T>{c.conv(v.a), c.conv(v.b)};
        }
    } else {
        for (int i = lane; i < pairs; i += 64) o2[i] = Two<T>{c.conv(s1[2 * i]), c.conv(s1[2 * i + 1])};
    }
    const int done = head + 2 * pairs;
    if (done < len && lane == 63) o[done] = c.conv(s[done]);
}

// One wave per destination row (destination d, plane z, row y); d is found in row0 by bisection.  The wave walks the
// row in segments: at x it scans the destination's box list from the last entry to the first for the first box that
// holds the voxel; the segment ends where that box ends, where a box scanned before it begins (it wins there), or
// -- with no box, when nothing is written -- where the next one begins.  All of that is wave-uniform (scalar loads
// and branches); only copy_segment() uses the lanes.
template <typename C>
__global__ __launch_bounds__(RG_THREADS) void scatter_boxes_kernel(
        const typename C::S* __restrict__ src, const BoxSrc* __restrict__ boxes, const BoxSrc* __restrict__ dsts,
        const unsigned long long* __restrict__ row0, int ndst, const int32_t* __restrict__ lists, int per_dst,
        unsigned long long rows, C c, typename C::T* __restrict__ pool) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long stride = (unsigned long long)gridDim.x * RG_WAVES;
    for (unsigned long long r = (unsigned long long)blockIdx.x * RG_WAVES + wave; r < rows; r += stride) {
        int lo = 0, hi = ndst - 1;                                    // the last d with row0[d] <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (row0[mid] <= r) lo = mid; else hi = mid - 1;
        }
        const BoxSrc& d = dsts[lo];
        const unsigned rem = (unsigned)(r - row0[lo]);
        const unsigned z = rem / (unsigned)d.ey, y = rem % (unsigned)d.ey;
        const long long pz = (long long)d.z0 + z, py = (long long)d.y0 + y;
        const int32_t* list = lists + (unsigned long long)lo * per_dst;
        typename C::T* orow = pool + d.base + (unsigned long long)z * d.stride_z + (unsigned long long)y * d.stride_y;
        const int ex = d.ex;
        int x = 0;
        while (x < ex) {
            const long long px = (long long)d.x0 + x;
            int len = ex - x;
            const typename C::S* s = nullptr;
            for (int j = per_dst - 1; j >= 0; j--) {
                const int k = list[j];
                if (k < 0) continue;
                const BoxSrc& b = boxes[k];
                if (pz < b.z0 || pz >= (long long)b.z0 + b.ez || py < b.y0 || py >= (long long)b.y0 + b.ey) continue;
                const long long x0 = b.x0, x1 = x0 + b.ex;
                if (px >= x0 && px < x1) {
                    if (x1 - px < len) len = (int)(x1 - px);
                    s = src + b.base + (unsigned long long)(pz - b.z0) * b.stride_z +
                        (unsigned long long)(py - b.y0) * b.stride_y + (unsigned long long)(px - x0);
                    break;
                }
                if (x0 > px && x0 - px < len) len = (int)(x0 - px);
            }
            if (s) copy_segment(c, orow + x, s, len, lane);
            x += len;
        }
    }
}

template <typename C>
static hipError_t scatter_launch(const void* src, const BoxSrc* boxes, const BoxSrc* dsts,
                                 const unsigned long long* row0, int ndst, const int32_t* lists, int per_dst,
                                 unsigned long long rows, C c, void* pool, hipStream_t s) {
    const unsigned long long want = (rows + RG_WAVES - 1) / RG_WAVES;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(scatter_boxes_kernel<C>, dim3(grid), dim3(RG_THREADS), 0, s,
                       static_cast<const typename C::S*>(src), boxes, dsts, row0, ndst, lists, per_dst, rows, c,
                       static_cast<typename C::T*>(pool));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_scatter_boxes(const void* src, int kind, const BoxSrc* boxes, const BoxSrc* dsts,
                                const unsigned long long* row0, int ndst, const int32_t* lists, int per_dst,
                                unsigned long long rows, float offset, void* pool, hipStream_t s) {
    if (rows == 0 || ndst == 0) return hipSuccess;
    if (kind == SCATTER_F32)
        return scatter_launch(src, boxes, dsts, row0, ndst, lists, per_dst, rows, CountsF32{offset}, pool, s);
    if (kind == SCATTER_U8)
        return scatter_launch(src, boxes, dsts, row0, ndst, lists, per_dst, rows, CopyU8{}, pool, s);
    return scatter_launch(src, boxes, dsts, row0, ndst, lists, per_dst, rows, CopyU16{}, pool, s);
}

hipError_t launch_gather_boxes(const uint16_t* pool, const BoxSrc* srcs, const int32_t* lists, int per_box,
                               const int32_t* starts, int nbox, int bz, int by, int bx, int out_f32, float offset,
                               float fill_f32, uint16_t fill_u16, void* out, hipStream_t s) {
    const unsigned long long rows = (unsigned long long)nbox * bz * by;
    if (rows == 0) return hipSuccess;
    const unsigned long long want = (rows + RG_WAVES - 1) / RG_WAVES;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    if (out_f32)
        hipLaunchKernelGGL(gather_boxes_kernel<PutF32>, dim3(grid), dim3(RG_THREADS), 0, s, pool, srcs, lists, per_box,
                           starts, rows, bz, by, bx, PutF32{fill_f32, offset}, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(gather_boxes_kernel<PutU16>, dim3(grid), dim3(RG_THREADS), 0, s, pool, srcs, lists, per_box,
                           starts, rows, bz, by, bx, PutU16{fill_u16}, static_cast<uint16_t*>(out));
    return hipGetLastError();
}

}  // namespace exabm4d
