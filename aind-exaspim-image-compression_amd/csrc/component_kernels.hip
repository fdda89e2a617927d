// component_kernels.hip -- the connected components of the seeds of a window and their filter by size (DESIGN.md
// 5.20, gfx950).  Four launches over the labelled REGION (the box grown by min_voxels - 1, cut at the volume):
//
//   1. cc_tile_kernel     a workgroup labels one tile of CC_TZ x CC_TY x CC_TX voxels by union-find in LDS and writes
//                         every seed's parent: the region index of the first voxel (raster order) of its component
//                         WITHIN THE TILE; other voxels get CC_NONE.
//   2. cc_merge_kernel    unites the seeds that face each other across tile faces, edges and corners.
//   3. cc_resolve_kernel  walks every seed to its root into a SEPARATE array (label = root + 1, background 0) and adds
//                         the sizes at the roots: one atomic per wave for the root of its first seed, one per run
//                         of equal roots for the others.
//   4. cc_filter_kernel   writes the seeds whose component has >= min_voxels voxels, and the three counters.
//
// A parent is only ever replaced by a SMALLER index of the same set (atomic min), so parent[v] <= v always, every
// walk along parents is strictly decreasing and ends, and the root of a set is its smallest index: the label is
// canonical, a pure function of the input.  No workgroup waits for another: there are no flags, tickets or spins,
// every loop is bounded by such a chain.
//
// Visibility: the per-XCD L2s are not coherent and an L1 is never refreshed by another CU's stores.  Launch 2 is the
// only one in which a workgroup reads entries another workgroup may change; there every access to `parent` is an
// agent-scope atomic (relaxed load, or fetch-min).  A stale parent would still be an ancestor of the same set, so the
// walk stays correct; the fetch-min returns the true old value.  Everything else crosses a kernel boundary.
#include <algorithm>

#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int CC_T = 256;
constexpr int CC_WAVES = CC_T / 64;
constexpr int CC_ROWS = CC_TZ * CC_TY;           // x rows of a tile, one wave wide
constexpr int CC_PER_WAVE = CC_ROWS / CC_WAVES;
constexpr uint32_t CC_NONE = 0xFFFFFFFFu;

static_assert(CC_TX == 64, "a row of a tile is one wave");
static_assert(CC_TZ == 8 && CC_TY == 8, "rows are split by shifts");

template <int SCOPE>
__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// Unites the sets of a and b.  Every value a parent ever held is <= its index, so all three loops strictly decrease.
template <int SCOPE>
__device__ __forceinline__ void cc_union(uint32_t* P, uint32_t a, uint32_t b) {
    for (uint32_t n = cc_load<SCOPE>(P + a); n != a; n = cc_load<SCOPE>(P + a)) a = n;
    for (uint32_t n = cc_load<SCOPE>(P + b); n != b; n = cc_load<SCOPE>(P + b)) b = n;
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);
        a = old == a ? b : old;                      // a was a root and now hangs under b; or go on from its parent
    }
}

// The rows (dz, dy) that precede a voxel's own in raster order: all four under 26-connectivity, (-1, 0) and (0, -1)
// under 6.  With the voxel before it in its own row they are the backward half of the neighbourhood.
__device__ __forceinline__ bool cc_row(int k, bool c26, int& dz, int& dy) {
    dz = k < 3 ? -1 : 0;
    dy = k < 3 ? k - 1 : -1;
    return c26 || k == 1 || k == 3;
}

template <typename T>
__global__ __launch_bounds__(CC_T) void cc_tile_kernel(const T* __restrict__ win, CcGeom g, uint32_t cut, int c26,
                                                       uint32_t* __restrict__ parent) {
    __shared__ uint32_t L[CC_ROWS * CC_TX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned tile = blockIdx.x;
    const int tx0 = (int)(tile % g.tiles[2]) * CC_TX;
    const int ty0 = (int)(tile / g.tiles[2] % g.tiles[1]) * CC_TY;
    const int tz0 = (int)(tile / g.tiles[2] / g.tiles[1]) * CC_TZ;
    const int x = tx0 + lane;                            // (region coordinates)

    // ---- seeds; a seed starts under the first voxel of its run along x (one ballot per row) ----
    uint32_t seeds = 0;
    for (int k = 0; k < CC_PER_WAVE; k++) {
        const int row = wave + k * CC_WAVES, z = tz0 + (row >> 3), y = ty0 + (row & 7);
        bool s = false;
        if (z < g.rd[0] && y < g.rd[1] && x < g.rd[2]) {
            const size_t i = ((size_t)(z + g.r0[0] - g.w0[0]) * g.wd[1] + (size_t)(y + g.r0[1] - g.w0[1])) *
                                 (size_t)g.wd[2] + (size_t)(x + g.r0[2] - g.w0[2]);
            s = (uint32_t)win[i] >= cut;
        }
        const unsigned long long m = __ballot(s);
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);
        const int start = below ? 64 - __clzll((long long)below) : 0;
        L[row * CC_TX + lane] = s ? (uint32_t)(row * CC_TX + start) : CC_NONE;
        seeds |= (uint32_t)s << k;
    }
    __syncthreads();

    // ---- the backward rows inside the tile.  Where the voxel straight across is a seed, the two beside it are in
    // its run (or joined to it by launch 2) and need no union of their own. ----
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    for (int k = 0; k < CC_PER_WAVE; k++) {
        if (!(seeds >> k & 1u)) continue;
        const int row = wave + k * CC_WAVES, lz = row >> 3, ly = row & 7;
        const uint32_t me = (uint32_t)(row * CC_TX + lane);
        for (int q = 0; q < 4; q++) {
            int dz, dy;
            if (!cc_row(q, c26 != 0, dz, dy)) continue;
            const int nz = lz + dz, ny = ly + dy;
            if (nz < 0 || ny < 0 || ny >= CC_TY) continue;
            const uint32_t n0 = (uint32_t)((nz * CC_TY + ny) * CC_TX + lane);
            if (cc_load<WG>(L + n0) != CC_NONE) {
                cc_union<WG>(L, me, n0);
            } else if (c26) {
                if (lane > 0 && cc_load<WG>(L + n0 - 1) != CC_NONE) cc_union<WG>(L, me, n0 - 1);
                if (lane < 63 && cc_load<WG>(L + n0 + 1) != CC_NONE) cc_union<WG>(L, me, n0 + 1);
            }
        }
    }
    __syncthreads();

    // ---- every seed to its root in the tile (nothing is written to LDS any more), as a region index ----
    for (int k = 0; k < CC_PER_WAVE; k++) {
        const int row = wave + k * CC_WAVES, z = tz0 + (row >> 3), y = ty0 + (row & 7);
        if (z >= g.rd[0] || y >= g.rd[1] || x >= g.rd[2]) continue;
        uint32_t out = CC_NONE;
        if (seeds >> k & 1u) {
            uint32_t r = L[row * CC_TX + lane];
            for (uint32_t n = L[r]; n != r; n = L[r]) r = n;
            const int rz = tz0 + (int)(r >> 9), ry = ty0 + (int)(r >> 6 & 7u), rx = tx0 + (int)(r & 63u);
            out = (uint32_t)(((long long)rz * g.rd[1] + ry) * g.rd[2] + rx);
        }
        parent[((long long)z * g.rd[1] + y) * g.rd[2] + x] = out;
    }
}

__global__ __launch_bounds__(CC_T) void cc_merge_kernel(CcGeom g, int c26, uint32_t* parent) {
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const long long idx = (long long)blockIdx.x * CC_T + threadIdx.x;
    if (idx >= g.voxels) return;
    const int x = (int)(idx % g.rd[2]), y = (int)(idx / g.rd[2] % g.rd[1]), z = (int)(idx / g.rd[2] / g.rd[1]);
    const int lx = x & (CC_TX - 1), ly = y & (CC_TY - 1), lz = z & (CC_TZ - 1);
    // only the shell of a tile has a neighbour in another tile
    if (lx != 0 && lx != CC_TX - 1 && ly != 0 && ly != CC_TY - 1 && lz != 0 && lz != CC_TZ - 1) return;
    const uint32_t me = (uint32_t)idx;
    if (cc_load<AG>(parent + me) == CC_NONE) return;
    if (x > 0 && lx == 0 && cc_load<AG>(parent + me - 1) != CC_NONE) cc_union<AG>(parent, me, me - 1);
    for (int q = 0; q < 4; q++) {
        int dz, dy;
        if (!cc_row(q, c26 != 0, dz, dy)) continue;
        const int nz = z + dz, ny = y + dy;
        if (nz < 0 || ny < 0 || ny >= g.rd[1]) continue;
        const bool other_row = (nz >> 3) != (z >> 3) || (ny >> 3) != (y >> 3);
        const uint32_t n0 = (uint32_t)(((long long)nz * g.rd[1] + ny) * g.rd[2] + x);
        if (cc_load<AG>(parent + n0) != CC_NONE) {
            if (other_row) cc_union<AG>(parent, me, n0);
        } else if (c26) {
            if (x > 0 && (other_row || lx == 0) && cc_load<AG>(parent + n0 - 1) != CC_NONE)
                cc_union<AG>(parent, me, n0 - 1);
            if (x + 1 < g.rd[2] && (other_row || lx == CC_TX - 1) && cc_load<AG>(parent + n0 + 1) != CC_NONE)
                cc_union<AG>(parent, me, n0 + 1);
        }
    }
}

__global__ __launch_bounds__(CC_T) void cc_resolve_kernel(CcGeom g, const uint32_t* __restrict__ parent,
                                                          uint32_t* __restrict__ labels,
                                                          uint32_t* __restrict__ sizes) {
    const long long idx = (long long)blockIdx.x * CC_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t r = CC_NONE;
    if (idx < g.voxels) {
        r = parent[idx];
        if (r != CC_NONE)
            for (uint32_t n = parent[r]; n != r; n = parent[r]) r = n;
        labels[idx] = r == CC_NONE ? 0u : r + 1u;
    }
    // The root of the wave's first seed gets one add for all its lanes, wherever they are (a large component has
    // many runs in a wave, and every add to its one counter is serial); the other roots one add per run of equal roots.
    const unsigned long long live = __ballot(r != CC_NONE);
    uint32_t key = r;
    if (live) {                                          // (wave-uniform)
        const int first = __ffsll((long long)live) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)r, first);
        const unsigned long long same = __ballot(r == lead);
        if (lane == first) atomicAdd(sizes + lead, (uint32_t)__popcll(same));
        if (r == lead) key = CC_NONE;
    }
    const uint32_t before = (uint32_t)__shfl_up((int)key, 1);
    const bool head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    if (head && key != CC_NONE) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : 64 - lane;
        atomicAdd(sizes + key, (uint32_t)run);
    }
}

__global__ __launch_bounds__(CC_T) void cc_filter_kernel(CcGeom g, uint32_t min_voxels,
                                                         const uint32_t* __restrict__ labels,
                                                         const uint32_t* __restrict__ sizes,
                                                         uint16_t* __restrict__ out16, uint8_t* __restrict__ out8,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned int red[3][CC_WAVES];
    const long long o = (long long)blockIdx.x * CC_T + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c[3] = {0u, 0u, 0u};                        // seeds, kept seeds, dropped components (first voxel here)
    if (o < g.box_voxels) {
        const int x = (int)(o % g.bd[2]) + g.b0[2], y = (int)(o / g.bd[2] % g.bd[1]) + g.b0[1],
                  z = (int)(o / g.bd[2] / g.bd[1]) + g.b0[0];                     // (volume coordinates)
        const long long idx = ((long long)(z - g.r0[0]) * g.rd[1] + (y - g.r0[1])) * g.rd[2] + (x - g.r0[2]);
        const uint32_t lab = labels[idx];
        const bool keep = lab != 0u && sizes[lab - 1u] >= min_voxels;
        if (out16) out16[o] = (uint16_t)keep;
        if (out8) out8[o] = (uint8_t)keep;
        if (z >= g.c0[0] && z < g.c0[0] + g.cd[0] && y >= g.c0[1] && y < g.c0[1] + g.cd[1] && x >= g.c0[2] &&
            x < g.c0[2] + g.cd[2]) {
            c[0] = lab != 0u;
            c[1] = keep;
            c[2] = lab == (uint32_t)idx + 1u && !keep;
        }
    }
    if (!counts) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned int n = (unsigned int)__popcll(__ballot(c[k] != 0u));
        if (lane == 0) red[k][wave] = n;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long t = 0ull;
        for (int w = 0; w < CC_WAVES; w++) t += red[threadIdx.x][w];
        if (t) atomicAdd(&counts[threadIdx.x], t);
    }
}

size_t components_scratch_bytes(long long voxels) {
    return 3 * (((size_t)voxels * sizeof(uint32_t) + 255) & ~(size_t)255);
}

bool components_geometry(const BoxGeom& b, const int* count0, const int* countd, long long grow, CcGeom& g) {
    g.voxels = g.box_voxels = 1;
    for (int a = 0; a < 3; a++) {
        g.w0[a] = b.w0[a];
        g.wd[a] = b.wd[a];
        g.b0[a] = b.b0[a];
        g.bd[a] = b.bd[a];
        g.c0[a] = count0[a];
        g.cd[a] = countd[a];
        g.r0[a] = (int)std::max(0ll, (long long)b.b0[a] - grow);
        g.rd[a] = (int)std::min((long long)b.n[a], (long long)b.b0[a] + b.bd[a] + grow) - g.r0[a];
        if (g.voxels > (1ll << 31) / g.rd[a]) return false;
        g.voxels *= g.rd[a];
        g.box_voxels *= g.bd[a];
    }
    g.tiles[0] = (unsigned)((g.rd[0] + CC_TZ - 1) / CC_TZ);
    g.tiles[1] = (unsigned)((g.rd[1] + CC_TY - 1) / CC_TY);
    g.tiles[2] = (unsigned)((g.rd[2] + CC_TX - 1) / CC_TX);
    return g.voxels < (1ll << 31);
}

hipError_t launch_components(const void* win, bool win_u8, const CcGeom& g, uint32_t cut, uint32_t min_voxels,
                             int connectivity, uint32_t* parent, uint32_t* labels, uint32_t* sizes, uint16_t* out16,
                             uint8_t* out8, unsigned long long* counts, hipStream_t s) {
    const int c26 = connectivity == 26;
    const unsigned tiles = g.tiles[0] * g.tiles[1] * g.tiles[2];      // < 2^31: every tile holds a voxel
    const unsigned blocks = (unsigned)((g.voxels + CC_T - 1) / CC_T);
    if (win_u8)
        hipLaunchKernelGGL(cc_tile_kernel<uint8_t>, dim3(tiles), dim3(CC_T), 0, s, static_cast<const uint8_t*>(win), g,
                           cut, c26, parent);
    else
        hipLaunchKernelGGL(cc_tile_kernel<uint16_t>, dim3(tiles), dim3(CC_T), 0, s, static_cast<const uint16_t*>(win),
                           g, cut, c26, parent);
    if (tiles > 1) hipLaunchKernelGGL(cc_merge_kernel, dim3(blocks), dim3(CC_T), 0, s, g, c26, parent);
    if (hipError_t e = hipMemsetAsync(sizes, 0, (size_t)g.voxels * sizeof(uint32_t), s)) return e;
    hipLaunchKernelGGL(cc_resolve_kernel, dim3(blocks), dim3(CC_T), 0, s, g, parent, labels, sizes);
    if (out16 || out8 || counts)
        hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)((g.box_voxels + CC_T - 1) / CC_T)), dim3(CC_T), 0, s, g,
                           min_voxels, labels, sizes, out16, out8, counts);
    return hipGetLastError();
}

}  // namespace exabm4d
