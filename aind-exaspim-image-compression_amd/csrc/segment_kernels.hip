// segment_kernels.hip -- the connected components of a whole volume from those of its bricks' windows (DESIGN.md 5.23,
// gfx950).  component_kernels.hip labels a WINDOW (a brick and one voxel more on the high side of every axis); the
// label of a component there is 1 + the window index of its first voxel.  Here:
//
//   collect  1. sg_collect_kernel  per voxel of the window: the own counts (the voxels of each component INSIDE THE
//                                  BRICK, added at the root's index), and the halo and face records -- (volume index,
//                                  provisional label) of the seeds outside the brick, and of the seeds of the brick on
//                                  a low face that another brick's window holds as halo.
//            2. sg_sizes_kernel    per root with an own count: the size record (provisional label, own count).  All are
//                                  counted; those below the capacity are stored.
//   relabel  1. sg_final_kernel    per root: one binary search of the sorted table by its provisional label into a
//                                  window-shaped array (the label itself where the table has no key).
//            2. sg_write_kernel    streams the brick: out = final[label - 1], background 0; 16 bytes per lane where the
//                                  addresses allow.
//
// A provisional label is the window label in volume coordinates, 64-bit: 1 + the volume index of the voxel at window
// index label - 1.  Records are appended with one atomic add per wave and record kind (ballot, popcount, the leader
// adds, every lane takes base + its rank), so their order is not determined; the host sorts them.  No workgroup
// waits for another and every loop is bounded (the binary search by 64 halvings).  Everything a launch reads that
// another wrote crosses a kernel boundary; the atomics are device-scope adds whose results only order the slots.
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int SG_T = 256;
constexpr uint32_t SG_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ void sg_coords(const SegGeom& g, uint32_t idx, int& z, int& y, int& x) {
    x = (int)(idx % (uint32_t)g.wd[2]);
    y = (int)(idx / (uint32_t)g.wd[2] % (uint32_t)g.wd[1]);
    z = (int)(idx / (uint32_t)g.wd[2] / (uint32_t)g.wd[1]);
}

// window coordinates -> the linear index in the volume
__device__ __forceinline__ unsigned long long sg_volume_index(const SegGeom& g, int z, int y, int x) {
    return ((unsigned long long)(z + g.w0[0]) * (unsigned long long)g.n[1] + (unsigned long long)(y + g.w0[1])) *
               (unsigned long long)g.n[2] + (unsigned long long)(x + g.w0[2]);
}

__device__ __forceinline__ unsigned long long sg_provisional(const SegGeom& g, uint32_t label) {
    int z, y, x;
    sg_coords(g, label - 1u, z, y, x);
    return 1ull + sg_volume_index(g, z, y, x);
}

// The slot of this lane's record: one add per wave.  Every lane of the wave calls it.
__device__ __forceinline__ unsigned long long sg_slot(bool want, unsigned long long* counter, int lane) {
    const unsigned long long m = __ballot(want);
    if (!m) return 0ull;                                 // (wave-uniform)
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0ull;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    return base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SG_T) void sg_collect_kernel(const uint32_t* __restrict__ labels, SegGeom g,
                                                          uint32_t* __restrict__ own, ulonglong2* __restrict__ halo,
                                                          unsigned long long halo_cap, ulonglong2* __restrict__ face,
                                                          unsigned long long face_cap,
                                                          unsigned long long* __restrict__ counts) {
    const long long idx = (long long)blockIdx.x * SG_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t lab = 0u;
    bool inside = false, low = false;
    int z = 0, y = 0, x = 0;
    if (idx < g.voxels) {
        lab = labels[idx];
        if (lab > (uint32_t)g.voxels) lab = 0u;          // (no labeller writes one; nothing is indexed past the window)
        sg_coords(g, (uint32_t)idx, z, y, x);
        const int vz = z + g.w0[0], vy = y + g.w0[1], vx = x + g.w0[2];
        inside = vz >= g.b0[0] && vz < g.b0[0] + g.bd[0] && vy >= g.b0[1] && vy < g.b0[1] + g.bd[1] &&
                 vx >= g.b0[2] && vx < g.b0[2] + g.bd[2];
        low = (vz == g.b0[0] && g.b0[0] > 0) || (vy == g.b0[1] && g.b0[1] > 0) || (vx == g.b0[2] && g.b0[2] > 0);
    }
    const bool seed = lab != 0u;

    // ---- own counts, as cc_resolve_kernel adds its sizes: the root of the wave's first own seed gets one add for
    // all its lanes, the other roots one add per run of equal roots ----
    const uint32_t r = seed && inside ? lab - 1u : SG_NONE;
    const unsigned long long live = __ballot(r != SG_NONE);
    uint32_t key = r;
    if (live) {                                          // (wave-uniform)
        const int first = __ffsll((long long)live) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)r, first);
        const unsigned long long same = __ballot(r == lead);
        if (lane == first) atomicAdd(own + lead, (uint32_t)__popcll(same));
        if (r == lead) key = SG_NONE;
    }
    const uint32_t before = (uint32_t)__shfl_up((int)key, 1);
    const bool head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    if (head && key != SG_NONE) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : 64 - lane;
        atomicAdd(own + key, (uint32_t)run);
    }

    // ---- halo and face records ----
    const bool is_halo = seed && !inside, is_face = seed && inside && low;
    const unsigned long long sh = sg_slot(is_halo, counts + 0, lane);
    const unsigned long long sf = sg_slot(is_face, counts + 1, lane);
    if (is_halo || is_face) {
        const ulonglong2 rec = make_ulonglong2(sg_volume_index(g, z, y, x), sg_provisional(g, lab));
        if (is_halo && sh < halo_cap) halo[sh] = rec;
        if (is_face && sf < face_cap) face[sf] = rec;
    }
}

__global__ __launch_bounds__(SG_T) void sg_sizes_kernel(const uint32_t* __restrict__ labels, SegGeom g,
                                                        const uint32_t* __restrict__ own,
                                                        ulonglong2* __restrict__ size, unsigned long long size_cap,
                                                        unsigned long long* __restrict__ counts) {
    const long long idx = (long long)blockIdx.x * SG_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t c = 0u;
    if (idx < g.voxels && labels[idx] == (uint32_t)idx + 1u) c = own[idx];
    const unsigned long long slot = sg_slot(c != 0u, counts + 2, lane);
    if (c != 0u && slot < size_cap)
        size[slot] = make_ulonglong2(sg_provisional(g, (uint32_t)idx + 1u), (unsigned long long)c);
}

template <typename T>
__global__ __launch_bounds__(SG_T) void sg_final_kernel(const uint32_t* __restrict__ labels, SegGeom g,
                                                        const unsigned long long* __restrict__ keys,
                                                        const unsigned long long* __restrict__ vals,
                                                        unsigned long long n_keys, T* __restrict__ final) {
    const long long idx = (long long)blockIdx.x * SG_T + threadIdx.x;
    if (idx >= g.voxels || labels[idx] != (uint32_t)idx + 1u) return;
    const unsigned long long prov = sg_provisional(g, (uint32_t)idx + 1u);
    unsigned long long lo = 0ull, hi = n_keys;           // the first key >= prov
    for (int it = 0; it < 64 && lo < hi; it++) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < prov) lo = mid + 1ull;
        else hi = mid;
    }
    final[idx] = (T)(lo < n_keys && keys[lo] == prov ? vals[lo] : prov);
}

template <typename T> struct SgVec;
template <> struct SgVec<uint32_t> { using type = uint4; };
template <> struct SgVec<unsigned long long> { using type = ulonglong2; };

template <typename T>
__global__ __launch_bounds__(SG_T) void sg_write_kernel(const uint32_t* __restrict__ labels, SegGeom g,
                                                        const T* __restrict__ final, T* __restrict__ out,
                                                        long long groups) {
    constexpr int V = 16 / (int)sizeof(T);               // voxels of a lane: 16 bytes of output
    using Vec = typename SgVec<T>::type;
    const long long t = (long long)blockIdx.x * SG_T + threadIdx.x;
    if (t >= groups) return;
    const int gx = (g.bd[2] + V - 1) / V;
    const int x0 = (int)(t % gx) * V, y = (int)(t / gx % g.bd[1]), z = (int)(t / gx / g.bd[1]);
    const int count = min(V, g.bd[2] - x0);
    const uint32_t* src = labels + ((long long)(z + g.b0[0] - g.w0[0]) * g.wd[1] + (y + g.b0[1] - g.w0[1])) * g.wd[2] +
                          (x0 + g.b0[2] - g.w0[2]);
    T* dst = out + ((long long)z * g.bd[1] + y) * g.bd[2] + x0;
    uint32_t lab[V];
    if (count == V && ((uintptr_t)src & (4 * V - 1)) == 0) {
        if constexpr (V == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            lab[0] = q.x, lab[1] = q.y, lab[2] = q.z, lab[3] = q.w;
        } else {
            const uint2 q = *reinterpret_cast<const uint2*>(src);
            lab[0] = q.x, lab[1] = q.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; j++) lab[j] = j < count ? src[j] : 0u;
    }
    T v[V];
#pragma unroll
    for (int j = 0; j < V; j++) v[j] = lab[j] && lab[j] <= (uint32_t)g.voxels ? final[lab[j] - 1u] : (T)0;
    if (count == V && ((uintptr_t)dst & 15) == 0) {
        Vec q;
        if constexpr (V == 4) q = make_uint4(v[0], v[1], v[2], v[3]);
        else q = make_ulonglong2(v[0], v[1]);
        *reinterpret_cast<Vec*>(dst) = q;
    } else {
#pragma unroll
        for (int j = 0; j < V; j++)
            if (j < count) dst[j] = v[j];
    }
}

long long segment_halo_records(const SegGeom& g) { return g.voxels - g.brick_voxels; }

long long segment_face_records(const SegGeom& g) {
    long long inner = 1;                                 // the voxels of the brick on none of those faces
    for (int a = 0; a < 3; a++) inner *= g.bd[a] - (g.b0[a] > 0 ? 1 : 0);
    return g.brick_voxels - inner;
}

hipError_t launch_segment_collect(const uint32_t* labels, const SegGeom& g, uint32_t* own, unsigned long long* halo,
                                  unsigned long long halo_cap, unsigned long long* face, unsigned long long face_cap,
                                  unsigned long long* size, unsigned long long size_cap, unsigned long long* counts,
                                  hipStream_t s) {
    const unsigned blocks = (unsigned)((g.voxels + SG_T - 1) / SG_T);
    hipLaunchKernelGGL(sg_collect_kernel, dim3(blocks), dim3(SG_T), 0, s, labels, g, own,
                       reinterpret_cast<ulonglong2*>(halo), halo_cap, reinterpret_cast<ulonglong2*>(face), face_cap,
                       counts);
    hipLaunchKernelGGL(sg_sizes_kernel, dim3(blocks), dim3(SG_T), 0, s, labels, g, own,
                       reinterpret_cast<ulonglong2*>(size), size_cap, counts);
    return hipGetLastError();
}

template <typename T>
static void sg_relabel(const uint32_t* labels, const SegGeom& g, const unsigned long long* keys,
                       const unsigned long long* vals, unsigned long long n_keys, T* final, T* out, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    const long long groups = (long long)g.bd[0] * g.bd[1] * ((g.bd[2] + V - 1) / V);
    hipLaunchKernelGGL(sg_final_kernel<T>, dim3((unsigned)((g.voxels + SG_T - 1) / SG_T)), dim3(SG_T), 0, s, labels, g,
                       keys, vals, n_keys, final);
    hipLaunchKernelGGL(sg_write_kernel<T>, dim3((unsigned)((groups + SG_T - 1) / SG_T)), dim3(SG_T), 0, s, labels, g,
                       final, out, groups);
}

hipError_t launch_segment_relabel(const uint32_t* labels, const SegGeom& g, const unsigned long long* keys,
                                  const unsigned long long* vals, unsigned long long n_keys, int typesize, void* final,
                                  void* out, hipStream_t s) {
    if (typesize == 4)
        sg_relabel<uint32_t>(labels, g, keys, vals, n_keys, static_cast<uint32_t*>(final), static_cast<uint32_t*>(out),
                             s);
    else
        sg_relabel<unsigned long long>(labels, g, keys, vals, n_keys, static_cast<unsigned long long*>(final),
                                       static_cast<unsigned long long*>(out), s);
    return hipGetLastError();
}

}  // namespace exabm4d
