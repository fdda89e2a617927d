// block_bounded_kernels.hip -- error-bounded lossy chunk codec with a ladder step per 8^3 block and a per-voxel bound
// (tests/block_bounded_pyref.py restates it from the oracle's dctq_forward / dctq_inverse and EXAC
// coder).  The arithmetic of a block is that of bounded_kernels.hip; what differs is who decides.
//
//   select:   one pass over the volume; a wave forward-transforms a block pair of one chunk once, then walks the
//             ladder from the coarsest step down: quantise, dequantise, invert, and compare |reconstruction - voxel|
//             with the voxel's own bound (max_error, or fg_max_error where the mask is set).  The two blocks get
//             separate wave-wide votes; a block's first admissible step on the way down is max A (the errors are
//             not monotone, so nothing is inferred from a failure).  The walk ends once both blocks have a verdict
//             -- the branch is wave-uniform.  A block belongs to one wave: its step goes straight into the chunk's
//             step plane and its indices at that step (its voxels if no step is admissible, zeros if it lies outside
//             the volume) into the chunk-major index volume, from the coefficients still in registers.
//             With a bound table the bound of a voxel is further capped by table[its value]: a
//             second instantiation gathers the 16 bounds of a lane once per pair and keeps them packed in registers.
//   assemble: per chunk the smaller of header + step plane + EXAC v2 of the indices and header + EXAC v2 of the
//             voxels, offsets by scan, everything copied 16 bytes at a time: the kernels are bq_assemble's
//             (bounded_pairs.h), this file states the format's policy (EbPolicy)
//   decode:   one wave per chunk validates offsets, header and step plane and lists the chunk for the EXAC decoder
//             of its mode; the inverse reads a step (or "verbatim") per block from the validated plane
#include "bounded_pairs.h"
#include "rans_common.h"

namespace exabm4d {

namespace {

constexpr uint32_t BB_VERBATIM = 0xFEu, BB_OUTSIDE = 0xFFu;
constexpr uint32_t BB_MAGIC = 'E' | ('B' << 8) | (1u << 16);       // magic, version 1; the mode is the fourth byte

// what bounds a voxel: max_error / fg_max_error, and with TABLE a device table of 65536 bounds indexed by its value
template <bool TABLE>
struct BbBound {
    float delta, delta_fg;
};
template <>
struct BbBound<true> {
    float delta, delta_fg;
    const uint16_t* table;
};

// waves_per_eu: left alone the compiler gives the table instantiation 131 VGPRs, three over what four waves per SIMD
// allow; a minimum of 1 is the default, so the other instantiation is what it was
template <bool TABLE>
__global__ __launch_bounds__(BQ_WAVES * 64) __attribute__((amdgpu_waves_per_eu(TABLE ? 4 : 1))) void
bb_select_kernel(const uint16_t* __restrict__ vol, const uint8_t* __restrict__ mask, BoundedGeom g, Dct7 T,
                 const float* __restrict__ qtab, int slices, BbBound<TABLE> bound, uint32_t nbp,
                 uint8_t* __restrict__ plane, int32_t* __restrict__ idx) {
    const float delta = bound.delta, delta_fg = bound.delta_fg;
    __shared__ __align__(16) float lds[BQ_WAVES * 2 * TBUF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hi = lane >> 3, lo = lane & 7;
    f2* tb = reinterpret_cast<f2*>(lds + wave * 2 * TBUF);
    const int c = blockIdx.x / slices, w = (blockIdx.x % slices) * BQ_WAVES + wave;
    const BqChunkBlocks cb = bq_chunk_blocks(g, c);
    // pairs of the chunk's NOMINAL block grid: every index and every plane byte of the chunk is written
    const int pairs_x = (g.cbx + 1) / 2, npairs = g.cbz * g.cby * pairs_x;
    int32_t* chunk_idx = idx + (size_t)c * g.nb * BVOX;
    uint8_t* pl = plane + (size_t)c * nbp;
    for (int p = w; p < npairs; p += slices * BQ_WAVES) {
        const PairAt at = pair_at(g, p, pairs_x, g.cby, g.cbx - 1);
        const bool two = at.lxb != at.lxa;              // an odd cbx ends on a duplicate: it never writes
        const bool live = at.lz < cb.lbz && at.ly < cb.lby;
        const bool ina = live && at.lxa < cb.lbx, inb = live && two && at.lxb < cb.lbx;
        // layout L3: lane = (ux, uy) = (hi, lo), registers = uz; coefficient index (uz, uy, ux)
        int32_t* oa = chunk_idx + (size_t)at.blka * BVOX + lo * 8 + hi;
        int32_t* ob = chunk_idx + (size_t)at.blkb * BVOX + lo * 8 + hi;
        if (!ina) {                     // then block b lies outside as well
#pragma unroll
            for (int u = 0; u < 8; u++) {
                oa[u * 64] = 0;
                if (two) ob[u * 64] = 0;
            }
            if (lane == 0) {
                pl[at.blka] = (uint8_t)BB_OUTSIDE;
                if (two) pl[at.blkb] = (uint8_t)BB_OUTSIDE;
            }
            continue;
        }
        const int bz = cb.bz0 + at.lz, by = cb.by0 + at.ly, bxa = cb.bx0 + at.lxa, bxb = cb.bx0 + at.lxb;
        f2 v[8], o[8];
        bq_load_pair(vol, g, bz, by, bxa, bxb, hi, lo, v);
#pragma unroll
        for (int y = 0; y < 8; y++) o[y] = v[y];
        // after pair_inv (no lane swap) lane (hi, lo) holds the voxels (z = hi, x = lo) again, registers = y.
        // Bit y of ina_y / inb_y: that voxel lies inside the volume; of fga / fgb: it is foreground.
        const int z = 8 * bz + hi, xa = 8 * bxa + lo, xb = 8 * bxb + lo;
        const bool oka = z < g.nz && xa < g.nx, okb = inb && z < g.nz && xb < g.nx;
        uint32_t ina_y = 0, inb_y = 0, fga = 0, fgb = 0;
        // TABLE: voxel y of block a / b in the low half of pa[y] / pb[y], its bound in the high half; these replace
        // o[] and the four bit sets in the walk, so the variant holds no more registers than the other.  The voxels
        // are exact in o[], edge replicas included, so every gather is in range; a voxel outside the volume gets
        // 65535, which no error of two uint16 exceeds, so it casts no vote.
        uint32_t pa[8], pb[8];
        if constexpr (TABLE) {
            const uint16_t* __restrict__ table = bound.table;
            const uint32_t d = (uint32_t)delta, dfg = (uint32_t)delta_fg;
            uint32_t ta[8], tb[8];
#pragma unroll
            for (int y = 0; y < 8; y++) {
                ta[y] = table[(uint32_t)o[y].x & 0xFFFFu];     // the mask changes no value: it lets the address be
                tb[y] = table[(uint32_t)o[y].y & 0xFFFFu];     // the table's base plus a 32-bit offset
            }
#pragma unroll
            for (int y = 0; y < 8; y++) {
                const int yy = 8 * by + y;
                uint32_t ba = 65535u, bb = 65535u;
                if (yy < g.ny) {
                    const size_t row = ((size_t)z * g.ny + yy) * g.nx;
                    if (oka) ba = min(ta[y], mask && mask[row + xa] ? dfg : d);
                    if (okb) bb = min(tb[y], mask && mask[row + xb] ? dfg : d);
                }
                pa[y] = (uint32_t)o[y].x | (ba << 16);
                pb[y] = (uint32_t)o[y].y | (bb << 16);
            }
        }
#pragma unroll
        for (int y = 0; y < 8; y++) {
            const int yy = 8 * by + y;
            if (!TABLE && yy < g.ny) {
                const size_t row = ((size_t)z * g.ny + yy) * g.nx;
                if (oka) {
                    ina_y |= 1u << y;
                    if (mask && mask[row + xa]) fga |= 1u << y;
                }
                if (okb) {
                    inb_y |= 1u << y;
                    if (mask && mask[row + xb]) fgb |= 1u << y;
                }
            }
        }
        pair_fwd(T, tb, hi, lo, v);
        int ja = -1, jb = -1;
        bool needa = true, needb = inb;
#pragma unroll 1
        for (int j = BQ_STEPS - 1; j >= 0; j--) {
            const float q = qtab[j];
            f2 r[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                r[u] = mk2((float)bq_quantise(v[u].x, q) * q, (float)bq_quantise(v[u].y, q) * q);
            pair_inv(T, tb, hi, lo, r);
            bool bada = false, badb = false;
#pragma unroll
            for (int y = 0; y < 8; y++) {
                if constexpr (TABLE) {
                    bada = bada || fabsf(bq_to_voxel(r[y].x) - (float)(pa[y] & 0xFFFFu)) > (float)(pa[y] >> 16);
                    badb = badb || fabsf(bq_to_voxel(r[y].y) - (float)(pb[y] & 0xFFFFu)) > (float)(pb[y] >> 16);
                } else {
                    const float ba = (fga >> y) & 1u ? delta_fg : delta, bb = (fgb >> y) & 1u ? delta_fg : delta;
                    bada = bada || (((ina_y >> y) & 1u) && fabsf(bq_to_voxel(r[y].x) - o[y].x) > ba);
                    badb = badb || (((inb_y >> y) & 1u) && fabsf(bq_to_voxel(r[y].y) - o[y].y) > bb);
                }
            }
            if (needa && __ballot(bada) == 0ull) {
                ja = j;
                needa = false;
            }
            if (needb && __ballot(badb) == 0ull) {
                jb = j;
                needb = false;
            }
            if (!needa && !needb) break;
        }
        // layout L1 of a verbatim block: slot (z * 8 + y) * 8 + x
        int32_t* ra = chunk_idx + (size_t)at.blka * BVOX + hi * 64 + lo;
        int32_t* rb = chunk_idx + (size_t)at.blkb * BVOX + hi * 64 + lo;
        if (ja >= 0) {
            const float q = qtab[ja];
#pragma unroll
            for (int u = 0; u < 8; u++) oa[u * 64] = bq_quantise(v[u].x, q);
        } else {
#pragma unroll
            for (int y = 0; y < 8; y++) ra[y * 8] = TABLE ? (int32_t)(pa[y] & 0xFFFFu) : (int32_t)o[y].x;
        }
        if (two) {
            if (!inb) {
#pragma unroll
                for (int u = 0; u < 8; u++) ob[u * 64] = 0;
            } else if (jb >= 0) {
                const float q = qtab[jb];
#pragma unroll
                for (int u = 0; u < 8; u++) ob[u * 64] = bq_quantise(v[u].y, q);
            } else {
#pragma unroll
                for (int y = 0; y < 8; y++) rb[y * 8] = TABLE ? (int32_t)(pb[y] & 0xFFFFu) : (int32_t)o[y].y;
            }
        }
        if (lane == 0) {
            pl[at.blka] = (uint8_t)(ja >= 0 ? (uint32_t)ja : BB_VERBATIM);
            if (two) pl[at.blkb] = (uint8_t)(!inb ? BB_OUTSIDE : jb >= 0 ? (uint32_t)jb : BB_VERBATIM);
        }
    }
}

// the "EB" streams to bq_assemble (bounded_pairs.h): mode 1 carries the chunk's padded step plane in front of the
// payload, and both modes two zero words in the header
struct EbPolicy {
    static constexpr uint32_t MAGIC = BB_MAGIC;
    uint32_t nbp;
    const uint8_t* plane;
    // mode 1 iff its stream (header, plane, indices) is strictly shorter than the mode-0 one (header, voxels)
    __device__ bool mode1(int c, const uint32_t* lossy_sz, const uint32_t* lossless_sz) const {
        return (unsigned long long)nbp + lossy_sz[c] < (unsigned long long)lossless_sz[c];
    }
    __device__ uint32_t word_y(int, bool) const { return 0u; }
    __device__ uint32_t word_z(int, bool) const { return 0u; }
    __device__ uint32_t prefix_bytes() const { return nbp; }
    __device__ const uint4* prefix(int c) const { return reinterpret_cast<const uint4*>(plane + (size_t)c * nbp); }
};

// one wave per chunk; status |= 64 for bad offsets, 32 for a bad header or step plane
__global__ __launch_bounds__(64) void bb_parse_kernel(const uint8_t* __restrict__ in, size_t in_bytes,
                                                      const unsigned long long* __restrict__ offsets, BoundedGeom g,
                                                      uint32_t nbp, uint32_t* __restrict__ mode,
                                                      uint32_t* __restrict__ lchunk,
                                                      unsigned long long* __restrict__ lrange,
                                                      uint32_t* __restrict__ lcount, uint32_t* __restrict__ status) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) mode[c] = 2u;        // neither: nothing is decoded for this chunk
    const unsigned long long o0 = offsets[c], o1 = offsets[c + 1];
    if (!bq_offsets_ok(o0, o1, in_bytes)) {
        if (lane == 0) atomicOr(status, 64u);
        return;
    }
    const uint4* h = reinterpret_cast<const uint4*>(in + o0);
    const uint4 a = h[0], b = h[1];
    const uint3 d = bq_shape_words(g, c);
    const uint32_t md = a.x >> 24;
    bool ok = (a.x & 0xFFFFFFu) == BB_MAGIC && md <= 1u && a.y == 0u && a.z == 0u && a.w == d.x && b.x == d.y &&
              b.y == d.z && b.z == 0u && b.w == 0u;
    ok = ok && (md == 0u || o1 - o0 >= (unsigned long long)BQ_HEADER + nbp);
    if (ok && md == 1u) {
        const BqChunkBlocks cb = bq_chunk_blocks(g, c);
        const uint8_t* pl = in + o0 + BQ_HEADER;
        bool bad = false;
        for (uint32_t i = (uint32_t)lane; i < nbp; i += 64u) {
            const uint32_t s = pl[i];
            if (i >= (uint32_t)g.nb) {
                bad = bad || s != 0u;                                      // padding
            } else {
                const int lx = (int)i % g.cbx, ly = ((int)i / g.cbx) % g.cby, lz = (int)i / (g.cbx * g.cby);
                const bool inside = lx < cb.lbx && ly < cb.lby && lz < cb.lbz;
                bad = bad || (inside ? !(s < (uint32_t)BQ_STEPS || s == BB_VERBATIM) : s != BB_OUTSIDE);
            }
        }
        ok = __ballot(bad) == 0ull;
    }
    if (!ok) {
        if (lane == 0) atomicOr(status, 32u);
        return;
    }
    if (lane == 0) bq_list_append(md, c, g.nchunks, o0 + BQ_HEADER + (md ? nbp : 0u), o1, mode, lchunk, lrange, lcount);
}

// the mode-1 chunks: every inside block at its own step, or copied; status |= 128 for a verbatim value that is no voxel
__global__ __launch_bounds__(BQ_WAVES * 64) void bb_inverse_kernel(const int32_t* __restrict__ idx,
                                                                   const uint8_t* __restrict__ in,
                                                                   const unsigned long long* __restrict__ offsets,
                                                                   BoundedGeom g, Dct7 T,
                                                                   const float* __restrict__ qtab,
                                                                   const uint32_t* __restrict__ mode, int slices,
                                                                   uint16_t* __restrict__ vol,
                                                                   uint32_t* __restrict__ status) {
    __shared__ __align__(16) float lds[BQ_WAVES * 2 * TBUF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hi = lane >> 3, lo = lane & 7;
    f2* tb = reinterpret_cast<f2*>(lds + wave * 2 * TBUF);
    const int c = blockIdx.x / slices, w = (blockIdx.x % slices) * BQ_WAVES + wave;
    if (mode[c] != 1u) return;
    const uint8_t* pl = in + offsets[c] + BQ_HEADER;    // validated by bb_parse_kernel
    const BqChunkBlocks cb = bq_chunk_blocks(g, c);
    const int pairs_x = (cb.lbx + 1) / 2, npairs = cb.lbz * cb.lby * pairs_x;
    const int32_t* chunk_idx = idx + (size_t)c * g.nb * BVOX;
    bool bad = false;
    for (int p = w; p < npairs; p += slices * BQ_WAVES) {
        const PairAt at = pair_at(g, p, pairs_x, cb.lby, cb.lbx - 1);
        const uint32_t sa = pl[at.blka], sb = pl[at.blkb];
        const bool va = sa == BB_VERBATIM, vb = sb == BB_VERBATIM;
        const int32_t* blka = chunk_idx + (size_t)at.blka * BVOX;
        const int32_t* blkb = chunk_idx + (size_t)at.blkb * BVOX;
        f2 v[8];
        if (!(va && vb)) {
            const float qa = va ? 0.0f : qtab[sa], qb = vb ? 0.0f : qtab[sb];
            const int32_t *ia = blka + lo * 8 + hi, *ib = blkb + lo * 8 + hi;
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = mk2((float)ia[u * 64] * qa, (float)ib[u * 64] * qb);
            pair_inv(T, tb, hi, lo, v);
        }
        const int z = 8 * (cb.bz0 + at.lz) + hi, xa = 8 * (cb.bx0 + at.lxa) + lo, xb = 8 * (cb.bx0 + at.lxb) + lo;
        const bool oka = z < g.nz && xa < g.nx, okb = at.lxb != at.lxa && z < g.nz && xb < g.nx;
#pragma unroll
        for (int y = 0; y < 8; y++) {
            const int yy = 8 * (cb.by0 + at.ly) + y;
            if (yy < g.ny) {
                const size_t row = ((size_t)z * g.ny + yy) * g.nx;
                if (oka) {
                    if (va) {
                        const int32_t r = blka[hi * 64 + y * 8 + lo];
                        bad = bad || r < 0 || r > 65535;
                        vol[row + xa] = (uint16_t)r;
                    } else {
                        vol[row + xa] = (uint16_t)(int)bq_to_voxel(v[y].x);
                    }
                }
                if (okb) {
                    if (vb) {
                        const int32_t r = blkb[hi * 64 + y * 8 + lo];
                        bad = bad || r < 0 || r > 65535;
                        vol[row + xb] = (uint16_t)r;
                    } else {
                        vol[row + xb] = (uint16_t)(int)bq_to_voxel(v[y].y);
                    }
                }
            }
        }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(status, 128u);
}

}  // namespace

uint32_t bb_plane_bytes(const BoundedGeom& g) { return ((uint32_t)g.nb + 15u) & ~15u; }

hipError_t launch_bb_select(const uint16_t* vol, const uint8_t* mask, const uint16_t* table, const BoundedGeom& g,
                            const float* dct64, const float* qtab, uint32_t delta, uint32_t delta_fg, uint8_t* plane,
                            int32_t* idx, hipStream_t s) {
    Dct7 T;
    unsigned grid;
    int slices;
    if (!bq_table(dct64, T) || !bq_grid(g, grid, slices)) return hipErrorInvalidValue;
    if (table)
        hipLaunchKernelGGL(bb_select_kernel<true>, dim3(grid), dim3(BQ_WAVES * 64), 0, s, vol, mask, g, T, qtab,
                           slices, BbBound<true>{(float)delta, (float)delta_fg, table}, bb_plane_bytes(g), plane, idx);
    else
        hipLaunchKernelGGL(bb_select_kernel<false>, dim3(grid), dim3(BQ_WAVES * 64), 0, s, vol, mask, g, T, qtab,
                           slices, BbBound<false>{(float)delta, (float)delta_fg}, bb_plane_bytes(g), plane, idx);
    return hipGetLastError();
}

hipError_t launch_bb_assemble(const BoundedGeom& g, const uint8_t* plane, const uint8_t* lossy,
                              const unsigned long long* lossy_off, const uint32_t* lossy_sz, const uint8_t* lossless,
                              const unsigned long long* lossless_off, const uint32_t* lossless_sz, uint32_t* sizes,
                              unsigned long long* offsets, unsigned long long* totals, uint8_t* out, hipStream_t s) {
    return bq_assemble(g, EbPolicy{bb_plane_bytes(g), plane}, BqStreams{lossy, lossy_off, lossy_sz},
                       BqStreams{lossless, lossless_off, lossless_sz}, sizes, offsets, totals, out, s);
}

hipError_t launch_bb_parse(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                           const BoundedGeom& g, uint32_t* mode, uint32_t* lchunk, unsigned long long* lrange,
                           uint32_t* lcount, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(bb_parse_kernel, dim3((unsigned)g.nchunks), dim3(64), 0, s, in, in_bytes, offsets, g,
                       bb_plane_bytes(g), mode, lchunk, lrange, lcount, status);
    return hipGetLastError();
}

hipError_t launch_bb_inverse(const int32_t* idx, const uint8_t* in, const unsigned long long* offsets,
                             const BoundedGeom& g, const float* dct64, const float* qtab, const uint32_t* mode,
                             uint16_t* vol, uint32_t* status, hipStream_t s) {
    Dct7 T;
    unsigned grid;
    int slices;
    if (!bq_table(dct64, T) || !bq_grid(g, grid, slices)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bb_inverse_kernel, dim3(grid), dim3(BQ_WAVES * 64), 0, s, idx, in, offsets, g, T, qtab, mode,
                       slices, vol, status);
    return hipGetLastError();
}

}  // namespace exabm4d
