// region_kernels.hip -- boxes gathered from a pool of decoded chunks: the read side of the chunk
// store.  A copy kernel: every output element is written once, every pool element a box covers is read once.
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

}  // namespace

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
