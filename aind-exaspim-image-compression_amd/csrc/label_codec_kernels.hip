// label_codec_kernels.hip -- the lossless label codec `exac-labels`: uint32 / uint64 volumes
// coded per 8^3 block as a sorted palette and packed indices, decoded whole, or read by boxes straight from the coded
// chunks.  One wave owns one block and one lane one x-row of 8 voxels; no workgroup waits for another: the encoder is
// a size pass, two scans and a write pass.
#include <algorithm>

#include "exabm4d_kernels.h"

namespace exabm4d {

namespace {

constexpr int LB_SLOTS = 512;            // voxels of a block
constexpr int LB_PALETTE = 256;          // most entries a palette holds

__host__ __device__ inline int ceil8(int v) { return (v + 7) >> 3; }

// Chunk c of the volume: origin, extent (truncated to the array) and its own block grid.
struct LbChunk {
    int z0, y0, x0, ez, ey, ex, ebz, eby, ebx, nblk;
};
__device__ inline LbChunk lb_chunk(const LabelGeom& g, int c) {
    LbChunk L;
    const int ix = c % g.gx, iy = (c / g.gx) % g.gy, iz = c / (g.gx * g.gy);
    L.z0 = iz * g.cz, L.y0 = iy * g.cy, L.x0 = ix * g.cx;
    L.ez = min(g.cz, g.nz - L.z0), L.ey = min(g.cy, g.ny - L.y0), L.ex = min(g.cx, g.nx - L.x0);
    L.ebz = ceil8(L.ez), L.eby = ceil8(L.ey), L.ebx = ceil8(L.ex);
    L.nblk = L.ebz * L.eby * L.ebx;
    return L;
}

// bits of a palette of k entries (1 <= k <= 256)
__host__ __device__ inline uint32_t lb_class(uint32_t k) { return k <= 1 ? 0u : k <= 2 ? 1u : k <= 4 ? 2u : k <= 16 ? 4u : 8u; }

// ---- encode ----------------------------------------------------------------------------------------------------
// One wave (= one workgroup, so __syncthreads() is the wave's own barrier) per block; lane = row z * 8 + y.
// WRITE = false: units[c * nb + b] <- the payload's size in 8-byte units.  WRITE = true: the table entry and the
// payload at blockoff[c * nb + b], and -- from the wave of block 0 -- the chunk's header.
template <typename T, bool WRITE>
__global__ __launch_bounds__(64) void label_encode_kernel(const T* __restrict__ vol, LabelGeom g,
                                                          uint32_t* __restrict__ units,
                                                          const uint32_t* __restrict__ blockoff,
                                                          const uint32_t* __restrict__ sizes,
                                                          const unsigned long long* __restrict__ offsets,
                                                          uint8_t* __restrict__ out) {
    __shared__ T keys[LB_SLOTS];
    __shared__ T pal[LB_PALETTE];
    const int lane = threadIdx.x;
    const int z = lane >> 3, y = lane & 7;
    const long long total = (long long)g.nchunks * g.nb;
    for (long long f = blockIdx.x; f < total; f += gridDim.x) {
        const int c = (int)(f / g.nb), b = (int)(f - (long long)c * g.nb);
        const LbChunk L = lb_chunk(g, c);
        if (b >= L.nblk) continue;                                  // a truncated chunk has fewer blocks
        const int bxi = b % L.ebx, byi = (b / L.ebx) % L.eby, bzi = b / (L.ebx * L.eby);
        const int pz = min(8, L.ez - 8 * bzi), py = min(8, L.ey - 8 * byi), px = min(8, L.ex - 8 * bxi);
        const bool row_present = z < pz && y < py;
        const T* blk = vol + ((size_t)(L.z0 + 8 * bzi) * g.ny + (size_t)(L.y0 + 8 * byi)) * g.nx + (L.x0 + 8 * bxi);
        const T first = blk[0];                                     // voxel (0, 0, 0) of a block is always present
        T v[8];
        if (row_present) {
            const T* src = blk + ((size_t)z * g.ny + y) * g.nx;
            if (px == 8 && (((uintptr_t)src) & 15) == 0) {
                const uint4* s4 = reinterpret_cast<const uint4*>(src);
                uint4 q[sizeof(T) / 2];
#pragma unroll
                for (int i = 0; i < (int)sizeof(T) / 2; i++) q[i] = s4[i];
                __builtin_memcpy(v, q, sizeof v);
            } else {
#pragma unroll
                for (int x = 0; x < 8; x++) v[x] = x < px ? src[x] : first;
            }
        } else {
#pragma unroll
            for (int x = 0; x < 8; x++) v[x] = first;               // absent voxels add no value to the set
        }
        bool same = true;
#pragma unroll
        for (int x = 0; x < 8; x++) same = same && v[x] == first;

        uint32_t k = 1;
        if (!__all(same)) {
            // the block's 512 keys sorted in LDS by a bitonic network: 45 steps of 256 compare-exchanges, 4 a lane
            __syncthreads();                                        // the last block's readers of keys / pal are done
#pragma unroll
            for (int x = 0; x < 8; x++) keys[lane * 8 + x] = v[x];
            __syncthreads();
            for (int size = 2; size <= LB_SLOTS; size <<= 1) {
                for (int j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int p = lane + 64 * t;
                        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                        const T a = keys[i], bb = keys[q];
                        const bool up = (i & size) == 0;
                        if ((a > bb) == up) {
                            keys[i] = bb;
                            keys[q] = a;
                        }
                    }
                    __syncthreads();
                }
            }
            // heads of runs -> palette positions by ballot and popcount
            k = 0;
            for (int j = 0; j < 8; j++) {
                const int i = j * 64 + lane;
                const T key = keys[i];
                const bool head = i == 0 || key != keys[i - 1];
                const unsigned long long m = __ballot(head);
                const uint32_t pos = k + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (head && pos < (uint32_t)LB_PALETTE) pal[pos] = key;
                k += (uint32_t)__popcll(m);
            }
            __syncthreads();
        }
        const bool raw = k > (uint32_t)LB_PALETTE;
        const uint32_t bits = raw ? 8u * (uint32_t)sizeof(T) : lb_class(k);
        const uint32_t pal_bytes = raw ? 0u : (k * (uint32_t)sizeof(T) + 7u) & ~7u;
        if (!WRITE) {
            if (lane == 0) units[f] = (pal_bytes + 64u * bits) >> 3;
            continue;
        }
        uint8_t* stream = out + offsets[c];
        if (b == 0 && lane == 0) {
            uint32_t* h = reinterpret_cast<uint32_t*>(stream);
            h[0] = LB_MAGIC;
            h[1] = 1u | ((uint32_t)sizeof(T) << 16);
            h[2] = (uint32_t)L.ez, h[3] = (uint32_t)L.ey, h[4] = (uint32_t)L.ex;
            h[5] = (uint32_t)L.nblk;
            h[6] = sizes[c];
            h[7] = 0u;
            if (sizes[c] & 8u) *reinterpret_cast<unsigned long long*>(stream + sizes[c]) = 0ull;   // the container's padding to 16
        }
        const uint32_t at = blockoff[f];
        if (lane == 0) reinterpret_cast<uint2*>(stream + LB_HEADER)[b] = make_uint2(at, (raw ? 0u : k) | (bits << 16));
        uint8_t* payload = stream + 8ull * at;
        if (raw) {
            T* o = reinterpret_cast<T*>(payload) + lane * 8;
#pragma unroll
            for (int x = 0; x < 8; x++) o[x] = (row_present && x < px) ? v[x] : (T)0;
            continue;
        }
        T* po = reinterpret_cast<T*>(payload);
        if (k == 1) {
            if (lane == 0) {
                po[0] = first;
                if (sizeof(T) == 4) po[1] = (T)0;
            }
            continue;
        }
        for (uint32_t i = lane; i < k; i += 64) po[i] = pal[i];
        if (sizeof(T) == 4 && (k & 1u) && lane == 0) po[k] = (T)0;       // the palette's padding to 8 bytes
        unsigned long long w = 0;
#pragma unroll
        for (int x = 0; x < 8; x++) {
            uint32_t lo = 0;                                        // the last entry <= v[x]: v[x] itself
#pragma unroll
            for (uint32_t step = LB_PALETTE / 2; step >= 1; step >>= 1)
                if (lo + step < k && pal[lo + step] <= v[x]) lo += step;
            if (row_present && x < px) w |= (unsigned long long)lo << (x * bits);
        }
        uint8_t* io = payload + pal_bytes + (uint32_t)lane * bits;  // a row is `bits` bytes, aligned to them
        if (bits == 1) *io = (uint8_t)w;
        else if (bits == 2) *reinterpret_cast<uint16_t*>(io) = (uint16_t)w;
        else if (bits == 4) *reinterpret_cast<uint32_t*>(io) = (uint32_t)w;
        else *reinterpret_cast<unsigned long long*>(io) = w;
    }
}

// One workgroup per chunk: blockoff[c * nb + b] = the payload's offset from the stream's start in 8-byte units
// (header, table, the payloads before it), sizes[c] = the stream's bytes.
__global__ __launch_bounds__(256) void label_scan_kernel(LabelGeom g, const uint32_t* __restrict__ units,
                                                         uint32_t* __restrict__ blockoff, uint32_t* __restrict__ sizes) {
    __shared__ uint32_t part[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const LbChunk L = lb_chunk(g, c);
    const size_t base = (size_t)c * g.nb;
    uint32_t run = (uint32_t)(LB_HEADER / 8) + (uint32_t)L.nblk;
    for (int b0 = 0; b0 < L.nblk; b0 += 256) {
        const int b = b0 + t;
        const uint32_t u = b < L.nblk ? units[base + b] : 0u;
        part[t] = u;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = t >= d ? part[t - d] : 0u;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (b < L.nblk) blockoff[base + b] = run + part[t] - u;
        run += part[255];
        __syncthreads();
    }
    if (t == 0) sizes[c] = 8u * run;
}

// ---- what the two decoders share: one block of a stream, opened under the stream's bounds ------------------------
struct LbBlock {
    const uint8_t* pal;      // the palette, or the raw values
    const uint8_t* idx;      // the index rows
    uint32_t k, bits;
    bool raw, ok;
};
// Entry b of the table of a stream of `sbytes` bytes whose table (nblk entries) the caller knows to lie inside it.
template <typename T>
__device__ inline LbBlock lb_open(const uint8_t* stream, unsigned long long sbytes, uint32_t nblk, uint32_t b) {
    LbBlock B;
    const uint2 e = reinterpret_cast<const uint2*>(stream + LB_HEADER)[b];
    B.k = e.y & 0xFFFFu;
    B.bits = (e.y >> 16) & 0xFFu;
    B.raw = B.bits == 8u * (uint32_t)sizeof(T);
    const unsigned long long at = 8ull * e.x, first = LB_HEADER + 8ull * nblk;
    unsigned long long pal_bytes = 0, need = (unsigned long long)LB_SLOTS * sizeof(T);
    B.ok = true;
    if (!B.raw) {
        B.ok = (B.bits == 0u || B.bits == 1u || B.bits == 2u || B.bits == 4u || B.bits == 8u) && B.k >= 1u &&
               B.k <= (1u << B.bits);
        pal_bytes = ((unsigned long long)B.k * sizeof(T) + 7ull) & ~7ull;
        need = pal_bytes + 64ull * B.bits;
    }
    B.ok = B.ok && at >= first && at + need <= sbytes;
    B.pal = stream + at;
    B.idx = B.pal + pal_bytes;
    return B;
}
// the `bits` bytes of index row `row`
__device__ inline unsigned long long lb_row_word(const LbBlock& B, int row) {
    switch (B.bits) {
        case 1: return B.idx[row];
        case 2: return reinterpret_cast<const uint16_t*>(B.idx)[row];
        case 4: return reinterpret_cast<const uint32_t*>(B.idx)[row];
        case 8: return reinterpret_cast<const unsigned long long*>(B.idx)[row];
        default: return 0ull;
    }
}
// voxel x of a row from its word: the index is clamped to k - 1 BEFORE the palette is read
template <typename T>
__device__ inline T lb_value(const LbBlock& B, unsigned long long w, int row, int x, bool& clamped) {
    if (B.raw) return reinterpret_cast<const T*>(B.pal)[row * 8 + x];
    uint32_t i = (uint32_t)(w >> (x * B.bits)) & ((1u << B.bits) - 1u);
    if (i >= B.k) {
        i = B.k - 1u;
        clamped = true;
    }
    return reinterpret_cast<const T*>(B.pal)[i];
}

// ---- decode of a whole volume: a wave per block, a lane per row -------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void label_decode_kernel(const uint8_t* __restrict__ in, unsigned long long in_bytes,
                                                           const unsigned long long* __restrict__ offsets, LabelGeom g,
                                                           T* __restrict__ vol, uint32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = lane >> 3, y = lane & 7;
    const long long total = (long long)g.nchunks * g.nb;
    for (long long f = (long long)blockIdx.x * 4 + wave; f < total; f += (long long)gridDim.x * 4) {
        const int c = (int)(f / g.nb), b = (int)(f - (long long)c * g.nb);
        const LbChunk L = lb_chunk(g, c);
        if (b >= L.nblk) continue;
        const int bxi = b % L.ebx, byi = (b / L.ebx) % L.eby, bzi = b / (L.ebx * L.eby);
        const int pz = min(8, L.ez - 8 * bzi), py = min(8, L.ey - 8 * byi), px = min(8, L.ex - 8 * bxi);
        const unsigned long long o0 = offsets[c], o1 = offsets[c + 1];
        const unsigned long long table_end = LB_HEADER + 8ull * (unsigned)L.nblk;
        bool ok = o0 <= o1 && o1 <= in_bytes && (o0 & 7ull) == 0ull && o1 - o0 >= table_end;
        const uint8_t* stream = in + o0;
        unsigned long long sbytes = 0;
        if (ok) {
            const uint32_t* h = reinterpret_cast<const uint32_t*>(stream);
            sbytes = h[6];
            ok = h[0] == LB_MAGIC && h[1] == (1u | ((uint32_t)sizeof(T) << 16)) && h[2] == (uint32_t)L.ez &&
                 h[3] == (uint32_t)L.ey && h[4] == (uint32_t)L.ex && h[5] == (uint32_t)L.nblk && sbytes >= table_end &&
                 sbytes <= o1 - o0;
        }
        LbBlock B{};
        if (ok) B = lb_open<T>(stream, sbytes, (uint32_t)L.nblk, (uint32_t)b);
        bool clamped = false;
        if (z < pz && y < py) {
            T* dst = vol + ((size_t)(L.z0 + 8 * bzi + z) * g.ny + (size_t)(L.y0 + 8 * byi + y)) * g.nx +
                     (L.x0 + 8 * bxi);
            T v[8];
            const unsigned long long w = B.ok && !B.raw ? lb_row_word(B, lane) : 0ull;
#pragma unroll
            for (int x = 0; x < 8; x++) v[x] = B.ok ? lb_value<T>(B, w, lane, x, clamped) : (T)0;
            if (px == 8 && (((uintptr_t)dst) & 15) == 0) {
                uint4 q[sizeof(T) / 2];
                __builtin_memcpy(q, v, sizeof v);
#pragma unroll
                for (int i = 0; i < (int)sizeof(T) / 2; i++) reinterpret_cast<uint4*>(dst)[i] = q[i];
            } else {
#pragma unroll
                for (int x = 0; x < 8; x++)
                    if (x < px) dst[x] = v[x];
            }
        }
        const uint32_t st = (B.ok ? 0u : LB_ST_MALFORMED) | (__any(clamped) ? LB_ST_CLAMPED : 0u);
        if (st && lane == 0) atomicOr(status, st);
    }
}

// ---- boxes straight from the coded chunks: a wave per output row, lanes along x ---------------------------------
struct LbGatherGeom {
    int nz, ny, nx, cz, cy, cx, bz, by, bx, per_box;
};
template <typename T>
__global__ __launch_bounds__(256) void label_gather_kernel(const uint8_t* __restrict__ data,
                                                           const LabelChunkSrc* __restrict__ srcs,
                                                           const int32_t* __restrict__ lists,
                                                           const int32_t* __restrict__ starts, unsigned long long rows,
                                                           LbGatherGeom g, T* __restrict__ out,
                                                           uint32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long stride = (unsigned long long)gridDim.x * 4;
    uint32_t st = 0;
    for (unsigned long long r = (unsigned long long)blockIdx.x * 4 + wave; r < rows; r += stride) {
        const unsigned long long n = r / ((unsigned long long)g.bz * g.by);
        const unsigned rem = (unsigned)(r - n * ((unsigned long long)g.bz * g.by));
        const long long sz = starts[3 * n], sy = starts[3 * n + 1], sx = starts[3 * n + 2];
        const long long pz = sz + rem / (unsigned)g.by, py = sy + rem % (unsigned)g.by;
        T* orow = out + r * (unsigned long long)g.bx;
        const bool row_inside = pz >= 0 && pz < g.nz && py >= 0 && py < g.ny && sx < g.nx && sx + g.bx > 0;
        // the box's chunk range (what the host laid its list out by) and this row's place in it
        int lx = 0, cnt_x = 1, row_at = 0, iz = 0, iy = 0;
        if (row_inside) {
            const int lz = (int)(max(sz, 0ll) / g.cz), ly = (int)(max(sy, 0ll) / g.cy);
            const int hy = (int)((min(sy + g.by, (long long)g.ny) - 1) / g.cy);
            lx = (int)(max(sx, 0ll) / g.cx);
            cnt_x = (int)((min(sx + g.bx, (long long)g.nx) - 1) / g.cx) - lx + 1;
            iz = (int)(pz / g.cz), iy = (int)(py / g.cy);
            row_at = ((iz - lz) * (hy - ly + 1) + (iy - ly)) * cnt_x;
        }
        const int32_t* list = lists + n * (unsigned long long)g.per_box;
        for (int x = lane; x < g.bx; x += 64) {
            const long long px = sx + x;
            T val = (T)0;
            if (row_inside && px >= 0 && px < g.nx) {
                const int ix = (int)(px / g.cx);
                const LabelChunkSrc& s = srcs[list[row_at + (ix - lx)]];
                const int qz = (int)(pz - s.z0), qy = (int)(py - s.y0), qx = (int)(px - s.x0);
                const int eby = ceil8(s.ey), ebx = ceil8(s.ex);
                const uint32_t nblk = (uint32_t)(ceil8(s.ez) * eby * ebx);
                const uint32_t b = (uint32_t)(((qz >> 3) * eby + (qy >> 3)) * ebx + (qx >> 3));
                const LbBlock B = lb_open<T>(data + s.offset, s.bytes, nblk, b);
                if (B.ok) {
                    const int row = (qz & 7) * 8 + (qy & 7);
                    bool clamped = false;
                    val = lb_value<T>(B, B.raw ? 0ull : lb_row_word(B, row), row, qx & 7, clamped);
                    if (clamped) st |= LB_ST_CLAMPED;
                } else {
                    st |= LB_ST_MALFORMED;
                }
            }
            orow[x] = val;
        }
    }
    if (st) atomicOr(status, st);
}

unsigned lb_grid(unsigned long long work, unsigned per_wg) {
    const unsigned long long wgs = (work + per_wg - 1) / per_wg;
    return (unsigned)std::min<unsigned long long>(std::max<unsigned long long>(wgs, 1), 1u << 20);
}

}  // namespace

int make_label_geom(int ts, int nz, int ny, int nx, int cz, int cy, int cx, LabelGeom& g) {
    if (ts != 4 && ts != 8) return 1;
    if (nz < 1 || ny < 1 || nx < 1 || cz < 1 || cy < 1 || cx < 1) return 1;
    if ((long long)nz * ny * nx > (1ll << 40)) return 1;
    g.ts = ts;
    g.nz = nz, g.ny = ny, g.nx = nx;
    g.cz = std::min(cz, nz), g.cy = std::min(cy, ny), g.cx = std::min(cx, nx);
    if ((long long)g.cz * g.cy * g.cx > (1ll << 27)) return 1;       // a stream stays below 2^31 bytes
    g.gz = (nz + g.cz - 1) / g.cz, g.gy = (ny + g.cy - 1) / g.cy, g.gx = (nx + g.cx - 1) / g.cx;
    const long long nchunks = (long long)g.gz * g.gy * g.gx;
    g.nb = ceil8(g.cz) * ceil8(g.cy) * ceil8(g.cx);
    if (nchunks > (1ll << 28) || nchunks * g.nb > (1ll << 30)) return 1;
    g.nchunks = (int)nchunks;
    return 0;
}

// every block raw, plus table and header, every stream padded to the container's 16 bytes
size_t label_volume_bound(const LabelGeom& g) {
    const size_t stream = LB_HEADER + (size_t)g.nb * (8 + (size_t)LB_SLOTS * g.ts);
    return (size_t)g.nchunks * ((stream + 15) & ~(size_t)15);
}

hipError_t launch_label_encode(const void* vol, const LabelGeom& g, uint32_t* units, uint32_t* blockoff, uint32_t* sizes,
                               unsigned long long* offsets, unsigned long long* totals, uint8_t* out, hipStream_t s) {
    const unsigned grid = lb_grid((unsigned long long)g.nchunks * g.nb, 1);
    if (g.ts == 4)
        hipLaunchKernelGGL((label_encode_kernel<uint32_t, false>), dim3(grid), dim3(64), 0, s,
                           static_cast<const uint32_t*>(vol), g, units, nullptr, nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL((label_encode_kernel<unsigned long long, false>), dim3(grid), dim3(64), 0, s,
                           static_cast<const unsigned long long*>(vol), g, units, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)g.nchunks), dim3(256), 0, s, g, units, blockoff, sizes);
    hipError_t e = launch_codec_scan(sizes, g.nchunks, offsets, totals, s);
    if (e != hipSuccess) return e;
    if (!out) return hipGetLastError();
    if (g.ts == 4)
        hipLaunchKernelGGL((label_encode_kernel<uint32_t, true>), dim3(grid), dim3(64), 0, s,
                           static_cast<const uint32_t*>(vol), g, units, blockoff, sizes, offsets, out);
    else
        hipLaunchKernelGGL((label_encode_kernel<unsigned long long, true>), dim3(grid), dim3(64), 0, s,
                           static_cast<const unsigned long long*>(vol), g, units, blockoff, sizes, offsets, out);
    return hipGetLastError();
}

hipError_t launch_label_decode(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets, const LabelGeom& g,
                               void* vol, uint32_t* status, hipStream_t s) {
    const unsigned grid = lb_grid((unsigned long long)g.nchunks * g.nb, 4);
    if (g.ts == 4)
        hipLaunchKernelGGL(label_decode_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, in, (unsigned long long)in_bytes,
                           offsets, g, static_cast<uint32_t*>(vol), status);
    else
        hipLaunchKernelGGL(label_decode_kernel<unsigned long long>, dim3(grid), dim3(256), 0, s, in,
                           (unsigned long long)in_bytes, offsets, g, static_cast<unsigned long long*>(vol), status);
    return hipGetLastError();
}

hipError_t launch_label_gather(const uint8_t* data, int ts, const LabelChunkSrc* srcs, const int32_t* lists, int per_box,
                               const int32_t* starts, int nbox, int bz, int by, int bx, const int* shape,
                               const int* chunk, void* out, uint32_t* status, hipStream_t s) {
    const unsigned long long rows = (unsigned long long)nbox * bz * by;
    if (!rows) return hipSuccess;
    const LbGatherGeom g{shape[0], shape[1], shape[2], chunk[0], chunk[1], chunk[2], bz, by, bx, per_box};
    const unsigned grid = lb_grid(rows, 4);
    if (ts == 4)
        hipLaunchKernelGGL(label_gather_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, data, srcs, lists, starts, rows, g,
                           static_cast<uint32_t*>(out), status);
    else
        hipLaunchKernelGGL(label_gather_kernel<unsigned long long>, dim3(grid), dim3(256), 0, s, data, srcs, lists,
                           starts, rows, g, static_cast<unsigned long long*>(out), status);
    return hipGetLastError();
}

}  // namespace exabm4d
