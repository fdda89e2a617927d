// bounded_pairs.h -- what the two error-bounded codecs share (bounded_kernels.hip: a step per chunk, DESIGN.md 3.10b;
// block_bounded_kernels.hip: a step per 8^3 block): the blocks of a chunk, the load of a block pair,
// the quantiser's rounding and the launch geometry; the E / C words of the 32-byte header, the assembly of the
// container (sizes, scan, header + payload copy) over a per-format policy, and the offsets check and list append of
// the parse kernels.  A wave owns a pair of x-adjacent blocks (dct_pairs.h).
#pragma once
#include "dct_pairs.h"
#include "exabm4d_kernels.h"

namespace exabm4d {

constexpr int BQ_WAVES = 4;
constexpr int BQ_PAIRS = 16;                 // block pairs per wave and workgroup (a chunk takes several workgroups)
constexpr float BQ_IDX_MAX = 1073741824.0f;  // indices are clamped to +-2^30

__device__ __forceinline__ int bq_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the blocks of chunk c: first block in the volume's block grid, and ceil(E / 8) blocks per axis inside the volume
struct BqChunkBlocks {
    int bz0, by0, bx0;
    int lbz, lby, lbx;
};
__device__ __forceinline__ BqChunkBlocks bq_chunk_blocks(const BoundedGeom& g, int c) {
    const int kx = c % g.gx, ky = (c / g.gx) % g.gy, kz = c / (g.gx * g.gy);
    BqChunkBlocks b;
    b.bz0 = kz * g.cbz;
    b.by0 = ky * g.cby;
    b.bx0 = kx * g.cbx;
    b.lbz = min(g.cbz, (g.nz - kz * g.cz + 7) / 8);
    b.lby = min(g.cby, (g.ny - ky * g.cy + 7) / 8);
    b.lbx = min(g.cbx, (g.nx - kx * g.cx + 7) / 8);
    return b;
}

// pair p of a block grid with pairs_x pairs a row and rows_y rows a plane (the chunk's nominal grid or its part inside
// the volume); last_x: the last block of a row, which an odd row length pairs with itself
struct PairAt {
    int lz, ly, lxa, lxb;       // block coordinates inside the chunk's nominal grid; lxb == lxa: no second block
    int blka, blkb;             // raster index in that grid
};
__device__ __forceinline__ PairAt pair_at(const BoundedGeom& g, int p, int pairs_x, int rows_y, int last_x) {
    const int px = p % pairs_x, t = p / pairs_x;
    PairAt a;
    a.ly = t % rows_y;
    a.lz = t / rows_y;
    a.lxa = 2 * px;
    a.lxb = min(2 * px + 1, last_x);
    a.blka = (a.lz * g.cby + a.ly) * g.cbx + a.lxa;
    a.blkb = (a.lz * g.cby + a.ly) * g.cbx + a.lxb;
    return a;
}

// layout L1 (lane = (z, x), registers = y) of two x-adjacent blocks, edge voxels replicated: dctq_forward_kernel's load
__device__ __forceinline__ void bq_load_pair(const uint16_t* __restrict__ vol, const BoundedGeom& g, int bz, int by,
                                             int bxa, int bxb, int hi, int lo, f2 (&v)[8]) {
    const size_t zrow = (size_t)bq_clamp(8 * bz + hi, 0, g.nz - 1) * g.ny;
    const int xa = bq_clamp(8 * bxa + lo, 0, g.nx - 1), xb = bq_clamp(8 * bxb + lo, 0, g.nx - 1);
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const size_t row = (zrow + bq_clamp(8 * by + y, 0, g.ny - 1)) * g.nx;
        v[y] = mk2((float)vol[row + xa], (float)vol[row + xb]);
    }
}

__device__ __forceinline__ int32_t bq_quantise(float c, float q) {
    return (int32_t)fminf(fmaxf(rintf(c / q), -BQ_IDX_MAX), BQ_IDX_MAX);
}

__device__ __forceinline__ float bq_to_voxel(float v) { return rintf(fminf(fmaxf(v, 0.0f), 65535.0f)); }

// workgroups per chunk so that a wave takes about BQ_PAIRS block pairs of a full chunk
inline int bq_slices(const BoundedGeom& g) {
    const long long pairs = (long long)g.cbz * g.cby * ((g.cbx + 1) / 2);
    const long long s = (pairs + BQ_WAVES * BQ_PAIRS - 1) / (BQ_WAVES * BQ_PAIRS);
    return (int)(s < 1 ? 1 : s);
}

inline bool bq_grid(const BoundedGeom& g, unsigned& grid, int& slices) {
    slices = bq_slices(g);
    const long long n = (long long)g.nchunks * slices;
    if (n > 0x7FFFFFFFll) return false;
    grid = (unsigned)n;
    return true;
}

inline bool bq_table(const float* dct64, Dct7& q7) {
    DctTable T;
    for (int i = 0; i < 64; i++) T.d[i] = dct64[i];
    return make_dct7(T, q7);
}

// ---- the 32-byte header's shape words, and the container's assembly ----------------------------------------------
__device__ __forceinline__ void chunk_extent(const BoundedGeom& g, int c, uint32_t& ez, uint32_t& ey, uint32_t& ex) {
    const int kx = c % g.gx, ky = (c / g.gx) % g.gy, kz = c / (g.gx * g.gy);
    ez = (uint32_t)min(g.cz, g.nz - kz * g.cz);
    ey = (uint32_t)min(g.cy, g.ny - ky * g.cy);
    ex = (uint32_t)min(g.cx, g.nx - kx * g.cx);
}

// header words 3, 4, 5 of chunk c in either format: its extent E, then the nominal chunk C (u16 each)
__device__ __forceinline__ uint3 bq_shape_words(const BoundedGeom& g, int c) {
    uint32_t ez, ey, ex;
    chunk_extent(g, c, ez, ey, ex);
    return make_uint3(ez | (ey << 16), ex | ((uint32_t)g.cz << 16), (uint32_t)g.cy | ((uint32_t)g.cx << 16));
}

// one candidate of every chunk as the chunk coder left it: container, offsets, exact sizes
struct BqStreams {
    const uint8_t* buf;
    const unsigned long long* off;
    const uint32_t* sz;
};

// A format's policy P (by value) says: MAGIC (magic and version; the mode is the fourth byte), mode1(c, lossy_sz,
// lossless_sz) -- is chunk c stored as mode 1 --, word_y / word_z(c, mode 1) -- header words 1 and 2 --,
// prefix_bytes() -- what a mode-1 stream holds between header and payload, a multiple of 16 -- and prefix(c), where
// that comes from (16-byte aligned).
template <class P>
__global__ __launch_bounds__(256) void bq_sizes_kernel(int nchunks, P pol, const uint32_t* __restrict__ lossy_sz,
                                                       const uint32_t* __restrict__ lossless_sz,
                                                       uint32_t* __restrict__ sizes) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    sizes[c] = (uint32_t)BQ_HEADER +
               (pol.mode1(c, lossy_sz, lossless_sz) ? pol.prefix_bytes() + lossy_sz[c] : lossless_sz[c]);
}

// one workgroup per chunk: header, (mode 1) the format's prefix, then the chosen payload; all 16-byte aligned in
// source and destination, and the source container's zero padding becomes the stream's
template <class P>
__global__ __launch_bounds__(256) void bq_copy_kernel(BoundedGeom g, P pol, BqStreams lossy, BqStreams lossless,
                                                      const unsigned long long* __restrict__ offsets,
                                                      uint8_t* __restrict__ out) {
    const int c = blockIdx.x;
    const bool lz = pol.mode1(c, lossy.sz, lossless.sz);
    uint4* dst = reinterpret_cast<uint4*>(out + offsets[c]);
    if (threadIdx.x == 0) {
        const uint3 d = bq_shape_words(g, c);
        dst[0] = make_uint4(P::MAGIC | ((lz ? 1u : 0u) << 24), pol.word_y(c, lz), pol.word_z(c, lz), d.x);
        dst[1] = make_uint4(d.y, d.z, 0u, 0u);
    }
    dst += 2;
    if (lz) {
        const uint4* pre = pol.prefix(c);
        for (uint32_t i = threadIdx.x; i < pol.prefix_bytes() / 16u; i += 256) dst[i] = pre[i];
        dst += pol.prefix_bytes() / 16u;
    }
    const BqStreams& from = lz ? lossy : lossless;
    const uint4* src = reinterpret_cast<const uint4*>(from.buf + from.off[c]);
    const uint32_t n16 = (from.sz[c] + 15u) / 16u;
    for (uint32_t i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

// mode per chunk from the two candidates' exact sizes, stream sizes, offsets by scan, then (out != NULL) the streams
template <class P>
hipError_t bq_assemble(const BoundedGeom& g, P pol, BqStreams lossy, BqStreams lossless, uint32_t* sizes,
                       unsigned long long* offsets, unsigned long long* totals, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(bq_sizes_kernel<P>, dim3((unsigned)((g.nchunks + 255) / 256)), dim3(256), 0, s, g.nchunks, pol,
                       lossy.sz, lossless.sz, sizes);
    hipError_t e = launch_codec_scan(sizes, g.nchunks, offsets, totals, s);
    if (e != hipSuccess || !out) return e;
    hipLaunchKernelGGL(bq_copy_kernel<P>, dim3((unsigned)g.nchunks), dim3(256), 0, s, g, pol, lossy, lossless, offsets,
                       out);
    return hipGetLastError();
}

// ---- what the two parse kernels share ---------------------------------------------------------------------------
// a chunk's stream lies inside the data, starts on 16 bytes and holds at least a header
__device__ __forceinline__ bool bq_offsets_ok(unsigned long long o0, unsigned long long o1, size_t in_bytes) {
    return !(o0 > o1 || o1 > in_bytes || (o0 & 15ull) || o1 - o0 < (unsigned long long)BQ_HEADER);
}

// chunk c joins the decode list of its mode with the payload [first, last) (one thread per chunk calls this)
__device__ __forceinline__ void bq_list_append(uint32_t md, int c, int nchunks, unsigned long long first,
                                               unsigned long long last, uint32_t* __restrict__ mode,
                                               uint32_t* __restrict__ lchunk, unsigned long long* __restrict__ lrange,
                                               uint32_t* __restrict__ lcount) {
    const uint32_t k = atomicAdd(lcount + md, 1u);
    lchunk[(size_t)md * nchunks + k] = (uint32_t)c;
    lrange[2 * ((size_t)md * nchunks + k)] = first;
    lrange[2 * ((size_t)md * nchunks + k) + 1] = last;
    mode[c] = md;
}

}  // namespace exabm4d
