// bounded_kernels.hip -- error-bounded lossy chunk codec (tests/bounded_pyref.py restates it
// from the oracle's dctq_forward / dctq_inverse and EXAC coder).
//
//   ladder:   one pass over the volume; every wave forward-transforms a block pair of one chunk once and, for
//             each of the 29 steps of the host's ladder table, quantises, dequantises, inverts and takes the
//             largest |reconstruction - voxel| over the voxels inside the volume: err[chunk][step] (atomicMax of
//             uint32, so the table does not depend on the order of the waves)
//   select:   j* = the largest step whose error is <= the bound, per chunk
//   forward:  indices at each chunk's own step, chunk-major: chunk c owns (nb, 8, 64) int32, zero outside the volume
//   assemble: per chunk the smaller of the lossy candidate (EXAC v2 of its indices) and the lossless one (EXAC v2
//             of its voxels), a 32-byte header in front, offsets by scan, payloads copied 16 bytes at a time: the
//             kernels are bq_assemble's (bounded_pairs.h), this file states the format's policy (EqPolicy)
//   decode:   parse + validate the headers (one thread per chunk) and list the chunks of either mode (the EXAC
//             decoder then walks each list), inverse transform of the lossy chunks at their own step
//
// The quantise / dequantise / inverse / clamp / round sequence is dctq_forward_kernel's followed by
// dctq_inverse_kernel's (codec_kernels.hip), with the seven-magnitude form of the DCT chains, which is
// bit-identical to the 64-entry table (dct_pairs.h): the error the ladder measures is the error every decoder
// produces.
#include "bounded_pairs.h"
#include "rans_common.h"

namespace exabm4d {

namespace {

__global__ __launch_bounds__(BQ_WAVES * 64) void bq_ladder_kernel(const uint16_t* __restrict__ vol, BoundedGeom g,
                                                                  Dct7 T, const float* __restrict__ qtab, int slices,
                                                                  uint32_t* __restrict__ err) {
    __shared__ __align__(16) float lds[BQ_WAVES * 2 * TBUF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hi = lane >> 3, lo = lane & 7;
    f2* tb = reinterpret_cast<f2*>(lds + wave * 2 * TBUF);
    const int c = blockIdx.x / slices, w = (blockIdx.x % slices) * BQ_WAVES + wave;
    const BqChunkBlocks cb = bq_chunk_blocks(g, c);
    // pairs inside the chunk: both blocks of a pair belong to chunk c
    const int pairs_x = (cb.lbx + 1) / 2, npairs = cb.lbz * cb.lby * pairs_x;
    uint32_t acc = 0;           // lane j < BQ_STEPS: largest error of step j over this wave's pairs
    for (int p = w; p < npairs; p += slices * BQ_WAVES) {
        const int px = p % pairs_x, t = p / pairs_x;
        const int by = cb.by0 + t % cb.lby, bz = cb.bz0 + t / cb.lby;
        const int bxa = cb.bx0 + 2 * px, bxb = cb.bx0 + min(2 * px + 1, cb.lbx - 1);
        f2 v[8], o[8];
        bq_load_pair(vol, g, bz, by, bxa, bxb, hi, lo, v);
#pragma unroll
        for (int y = 0; y < 8; y++) o[y] = v[y];
        pair_fwd(T, tb, hi, lo, v);
        // after pair_inv (no lane swap) lane (hi, lo) holds the voxels (z = hi, x = lo) again, registers = y
        const bool zin = 8 * bz + hi < g.nz;
        const bool oka = zin && 8 * bxa + lo < g.nx, okb = zin && 8 * bxb + lo < g.nx;
        const int yv = g.ny - 8 * by;
#pragma unroll 1
        for (int j = 0; j < BQ_STEPS; j++) {
            const float q = qtab[j];
            f2 r[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                r[u] = mk2((float)bq_quantise(v[u].x, q) * q, (float)bq_quantise(v[u].y, q) * q);
            pair_inv(T, tb, hi, lo, r);
            float m = 0.0f;
#pragma unroll
            for (int y = 0; y < 8; y++) {
                if (y < yv) {
                    if (oka) m = fmaxf(m, fabsf(bq_to_voxel(r[y].x) - o[y].x));
                    if (okb) m = fmaxf(m, fabsf(bq_to_voxel(r[y].y) - o[y].y));
                }
            }
            const uint32_t mw = wave_max((uint32_t)m);
            if (lane == j) acc = max(acc, mw);
        }
    }
    if (lane < BQ_STEPS && acc) atomicMax(err + (size_t)c * BQ_STEPS + lane, acc);
}

__global__ __launch_bounds__(256) void bq_select_kernel(const uint32_t* __restrict__ err, int nchunks, uint32_t delta,
                                                        const float* __restrict__ qtab, int32_t* __restrict__ jsel,
                                                        float* __restrict__ qsel) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    int j = -1;
    for (int k = 0; k < BQ_STEPS; k++)
        if (err[(size_t)c * BQ_STEPS + k] <= delta) j = k;
    jsel[c] = j;
    qsel[c] = j >= 0 ? qtab[j] : 0.0f;
}

__global__ __launch_bounds__(BQ_WAVES * 64) void bq_forward_kernel(const uint16_t* __restrict__ vol, BoundedGeom g,
                                                                   Dct7 T, const float* __restrict__ qsel, int slices,
                                                                   int32_t* __restrict__ idx) {
    __shared__ __align__(16) float lds[BQ_WAVES * 2 * TBUF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hi = lane >> 3, lo = lane & 7;
    f2* tb = reinterpret_cast<f2*>(lds + wave * 2 * TBUF);
    const int c = blockIdx.x / slices, w = (blockIdx.x % slices) * BQ_WAVES + wave;
    const BqChunkBlocks cb = bq_chunk_blocks(g, c);
    const float q = qsel[c];
    // pairs of the chunk's NOMINAL block grid: every index of the chunk is written
    const int pairs_x = (g.cbx + 1) / 2, npairs = g.cbz * g.cby * pairs_x;
    int32_t* base = idx + (size_t)c * g.nb * BVOX + lo * 8 + hi;
    for (int p = w; p < npairs; p += slices * BQ_WAVES) {
        const int px = p % pairs_x, t = p / pairs_x;
        const int ly = t % g.cby, lz = t / g.cby;
        const int lxa = 2 * px, lxb = min(2 * px + 1, g.cbx - 1);
        const bool live = q > 0.0f && lz < cb.lbz && ly < cb.lby;
        const bool ina = live && lxa < cb.lbx, inb = live && lxb < cb.lbx;
        // layout L3: lane = (ux, uy) = (hi, lo), registers = uz; coefficient index (uz, uy, ux)
        int32_t* oa = base + ((size_t)(lz * g.cby + ly) * g.cbx + lxa) * BVOX;
        int32_t* ob = base + ((size_t)(lz * g.cby + ly) * g.cbx + lxb) * BVOX;
        if (!ina) {                     // then block b lies outside as well
#pragma unroll
            for (int u = 0; u < 8; u++) {
                oa[u * 64] = 0;
                if (lxb != lxa) ob[u * 64] = 0;
            }
            continue;
        }
        f2 v[8];
        bq_load_pair(vol, g, cb.bz0 + lz, cb.by0 + ly, cb.bx0 + lxa, cb.bx0 + lxb, hi, lo, v);
        pair_fwd(T, tb, hi, lo, v);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            oa[u * 64] = bq_quantise(v[u].x, q);
            if (lxb != lxa) ob[u * 64] = inb ? bq_quantise(v[u].y, q) : 0;
        }
    }
}

constexpr uint32_t BQ_MAGIC = 'E' | ('Q' << 8) | (1u << 16);       // magic, version 1; the mode is the fourth byte

// the "EQ" streams to bq_assemble (bounded_pairs.h): mode 1 carries j* and q in the header and nothing in front of
// the payload
struct EqPolicy {
    static constexpr uint32_t MAGIC = BQ_MAGIC;
    const int32_t* jsel;
    const float* qsel;
    __device__ bool mode1(int c, const uint32_t* lossy_sz, const uint32_t* lossless_sz) const {
        return jsel[c] >= 0 && lossy_sz[c] < lossless_sz[c];        // a tie goes to the lossless stream
    }
    // j* and three zero bytes, then q (float32 bits)
    __device__ uint32_t word_y(int c, bool lz) const { return lz ? (uint32_t)jsel[c] : 0xFFu; }
    __device__ uint32_t word_z(int c, bool lz) const { return lz ? __float_as_uint(qsel[c]) : 0u; }
    __device__ uint32_t prefix_bytes() const { return 0u; }
    __device__ const uint4* prefix(int) const { return nullptr; }
};

__global__ __launch_bounds__(256) void bq_parse_kernel(const uint8_t* __restrict__ in, size_t in_bytes,
                                                       const unsigned long long* __restrict__ offsets, BoundedGeom g,
                                                       const float* __restrict__ qtab, uint32_t* __restrict__ mode,
                                                       float* __restrict__ qv, uint32_t* __restrict__ lchunk,
                                                       unsigned long long* __restrict__ lrange,
                                                       uint32_t* __restrict__ lcount, uint32_t* __restrict__ status) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.nchunks) return;
    mode[c] = 2u;                       // neither: nothing is decoded for this chunk
    qv[c] = 0.0f;
    const unsigned long long o0 = offsets[c], o1 = offsets[c + 1];
    if (!bq_offsets_ok(o0, o1, in_bytes)) {
        atomicOr(status, 64u);
        return;
    }
    const uint4* h = reinterpret_cast<const uint4*>(in + o0);
    const uint4 a = h[0], b = h[1];
    const uint3 d = bq_shape_words(g, c);
    const uint32_t md = a.x >> 24, j = a.y & 0xFFu;
    bool ok = (a.x & 0xFFFFFFu) == BQ_MAGIC;
    if (md == 0u)
        ok = ok && j == 0xFFu && a.z == 0u;
    else if (md == 1u)
        ok = ok && j < (uint32_t)BQ_STEPS && a.z == __float_as_uint(qtab[min(j, (uint32_t)BQ_STEPS - 1u)]);
    else
        ok = false;
    ok = ok && a.w == d.x && b.x == d.y && b.y == d.z;
    if (!ok) {
        atomicOr(status, 32u);
        return;
    }
    bq_list_append(md, c, g.nchunks, o0 + BQ_HEADER, o1, mode, lchunk, lrange, lcount);
    qv[c] = md ? __uint_as_float(a.z) : 0.0f;
}

__global__ __launch_bounds__(BQ_WAVES * 64) void bq_inverse_kernel(const int32_t* __restrict__ idx, BoundedGeom g,
                                                                   Dct7 T, const uint32_t* __restrict__ mode,
                                                                   const float* __restrict__ qv, int slices,
                                                                   uint16_t* __restrict__ vol) {
    __shared__ __align__(16) float lds[BQ_WAVES * 2 * TBUF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hi = lane >> 3, lo = lane & 7;
    f2* tb = reinterpret_cast<f2*>(lds + wave * 2 * TBUF);
    const int c = blockIdx.x / slices, w = (blockIdx.x % slices) * BQ_WAVES + wave;
    if (mode[c] != 1u) return;
    const float q = qv[c];
    const BqChunkBlocks cb = bq_chunk_blocks(g, c);
    const int pairs_x = (cb.lbx + 1) / 2, npairs = cb.lbz * cb.lby * pairs_x;
    const int32_t* base = idx + (size_t)c * g.nb * BVOX + lo * 8 + hi;
    for (int p = w; p < npairs; p += slices * BQ_WAVES) {
        const PairAt at = pair_at(g, p, pairs_x, cb.lby, cb.lbx - 1);
        const int ly = at.ly, lz = at.lz, lxa = at.lxa, lxb = at.lxb;
        const int32_t* ia = base + ((size_t)(lz * g.cby + ly) * g.cbx + lxa) * BVOX;
        const int32_t* ib = base + ((size_t)(lz * g.cby + ly) * g.cbx + lxb) * BVOX;
        f2 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = mk2((float)ia[u * 64] * q, (float)ib[u * 64] * q);
        pair_inv(T, tb, hi, lo, v);
        const int z = 8 * (cb.bz0 + lz) + hi, xa = 8 * (cb.bx0 + lxa) + lo, xb = 8 * (cb.bx0 + lxb) + lo;
#pragma unroll
        for (int y = 0; y < 8; y++) {
            const int yy = 8 * (cb.by0 + ly) + y;
            if (z < g.nz && yy < g.ny) {
                const size_t row = ((size_t)z * g.ny + yy) * g.nx;
                if (xa < g.nx) vol[row + xa] = (uint16_t)(int)bq_to_voxel(v[y].x);
                if (lxb != lxa && xb < g.nx) vol[row + xb] = (uint16_t)(int)bq_to_voxel(v[y].y);
            }
        }
    }
}

}  // namespace

int make_bounded_geom(int nz, int ny, int nx, int cz, int cy, int cx, BoundedGeom& g) {
    if (nz < 1 || ny < 1 || nx < 1) return -1;
    if (cz < 8 || cy < 8 || cx < 8 || (cz | cy | cx) & 7 || cz > 65535 || cy > 65535 || cx > 65535) return -1;
    const unsigned long long cn = (unsigned long long)cz * cy * cx;
    if (cn > (1ull << 28)) return -1;                   // the chunk coder's limit (make_codec_geom)
    g.nz = nz; g.ny = ny; g.nx = nx;
    g.cz = cz; g.cy = cy; g.cx = cx;
    g.gz = (nz + cz - 1) / cz;
    g.gy = (ny + cy - 1) / cy;
    g.gx = (nx + cx - 1) / cx;
    const unsigned long long nchunks = (unsigned long long)g.gz * g.gy * g.gx;
    g.cbz = cz / 8; g.cby = cy / 8; g.cbx = cx / 8;
    g.nb = g.cbz * g.cby * g.cbx;
    // the index volume (nchunks * nb, 8, 64) is one chunk-coder volume: its z extent is an int
    if (nchunks > 0x7FFFFFFFull || nchunks * (unsigned long long)g.nb > 0x7FFFFFFFull) return -1;
    g.nchunks = (int)nchunks;
    return 0;
}

hipError_t launch_bq_ladder(const uint16_t* vol, const BoundedGeom& g, const float* dct64, const float* qtab,
                            uint32_t* err, hipStream_t s) {
    Dct7 T;
    unsigned grid;
    int slices;
    if (!bq_table(dct64, T) || !bq_grid(g, grid, slices)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bq_ladder_kernel, dim3(grid), dim3(BQ_WAVES * 64), 0, s, vol, g, T, qtab, slices, err);
    return hipGetLastError();
}

hipError_t launch_bq_select(const uint32_t* err, int nchunks, uint32_t delta, const float* qtab, int32_t* jsel,
                            float* qsel, hipStream_t s) {
    hipLaunchKernelGGL(bq_select_kernel, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s, err, nchunks, delta,
                       qtab, jsel, qsel);
    return hipGetLastError();
}

hipError_t launch_bq_forward(const uint16_t* vol, const BoundedGeom& g, const float* dct64, const float* qsel,
                             int32_t* idx, hipStream_t s) {
    Dct7 T;
    unsigned grid;
    int slices;
    if (!bq_table(dct64, T) || !bq_grid(g, grid, slices)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bq_forward_kernel, dim3(grid), dim3(BQ_WAVES * 64), 0, s, vol, g, T, qsel, slices, idx);
    return hipGetLastError();
}

hipError_t launch_bq_assemble(const BoundedGeom& g, const int32_t* jsel, const float* qsel,
                              const uint8_t* lossy, const unsigned long long* lossy_off, const uint32_t* lossy_sz,
                              const uint8_t* lossless, const unsigned long long* lossless_off,
                              const uint32_t* lossless_sz, uint32_t* sizes, unsigned long long* offsets,
                              unsigned long long* totals, uint8_t* out, hipStream_t s) {
    return bq_assemble(g, EqPolicy{jsel, qsel}, BqStreams{lossy, lossy_off, lossy_sz},
                       BqStreams{lossless, lossless_off, lossless_sz}, sizes, offsets, totals, out, s);
}

hipError_t launch_bq_parse(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                           const BoundedGeom& g, const float* qtab, uint32_t* mode, float* qv, uint32_t* lchunk,
                           unsigned long long* lrange, uint32_t* lcount, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(bq_parse_kernel, dim3((unsigned)((g.nchunks + 255) / 256)), dim3(256), 0, s, in, in_bytes,
                       offsets, g, qtab, mode, qv, lchunk, lrange, lcount, status);
    return hipGetLastError();
}

hipError_t launch_bq_inverse(const int32_t* idx, const BoundedGeom& g, const float* dct64, const uint32_t* mode,
                             const float* qv, uint16_t* vol, hipStream_t s) {
    Dct7 T;
    unsigned grid;
    int slices;
    if (!bq_table(dct64, T) || !bq_grid(g, grid, slices)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bq_inverse_kernel, dim3(grid), dim3(BQ_WAVES * 64), 0, s, idx, g, T, mode, qv, slices, vol);
    return hipGetLastError();
}

}  // namespace exabm4d
