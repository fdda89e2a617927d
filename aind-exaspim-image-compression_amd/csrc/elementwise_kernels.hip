// elementwise_kernels.hip -- HBM-bound streams of the hot path:
//   normalise (a-B6) + clip (a-C)                  data_handling.py:333
//   u16 -> f32 - offset (a-A)                      data_handling.py:353-354
//   intensity transforms forward / inverse (a-D/E) transforms.py:113-152, :223-285, :332-371, :398-411
//   overlap-tile gather / accumulate / finalise    inference.py:81-116, :153-199
// Checker: oracle/host_oracle.py (pinned by tests/golden/*.npz generated from the reference).
//
// fp32 rounding points follow numpy: every Python-float constant of the reference object is
// rounded to fp32 where numpy rounds it (host side, TfDev below) and every array operation is one
// fp32 operation here (-ffp-contract=off; no fused multiply-add).  arcsinh / sinh are evaluated in
// fp64 and rounded once.
#include <algorithm>

#include "exabm4d_kernels.h"

namespace exabm4d {


__device__ __forceinline__ float tf_forward(const TfDev& t, float x) {
    if (t.wrapped) x = x - t.woff;
    if (t.kind == 0) {
        const float u = (x - t.off) / t.scale;
        const float a = (float)asinh((double)u);
        return a / t.norm;
    } else if (t.kind == 1) {
        float arg = t.gain * (x - t.off);
        arg = arg + t.c38g2;
        arg = arg + t.rn2;
        const float g = t.two_over_gain * sqrtf(fmaxf(arg, 0.0f));
        return g / t.norm;
    } else {
        const float y = (x - t.mn) / t.fden;
        return fminf(fmaxf(y, 0.0f), t.clip);
    }
}
__device__ __forceinline__ float tf_inverse_float(const TfDev& t, float y) {
    float c;
    if (t.kind == 0) {
        const float s = (float)sinh((double)(y * t.norm));
        c = t.off + t.scale * s;
    } else if (t.kind == 1) {
        const float d = fmaxf(y, 0.0f) * t.norm;
        const float h = d * t.gain / 2.0f;
        const float arg = h * h;
        const float u = (arg - t.cinvg2) - t.rn2;
        c = t.off + u / t.gain;
    } else {
        c = y * t.range + t.mn;
    }
    if (t.wrapped) c = c + t.woff;
    return c;
}
__device__ __forceinline__ uint16_t quantise_u16(float c, float maxc) {
    c = fminf(fmaxf(c, 0.0f), maxc);     // np.clip(counts, 0, max_count)
    return (uint16_t)rintf(c);           // np.rint (half-to-even) then astype(uint16)
}

// Poisson-Gaussian stabilisation (tests/pg_pyref.py states the operation order).  The forward is
// tf_forward kind 1 without the division by norm: unit noise sigma in D.
__device__ __forceinline__ float pg_forward(const PgDev& t, float x) {
    float a = t.gain * (x - t.off);
    a = a + t.c38g2;
    a = a + t.rn2;
    return t.two_over_gain * sqrtf(fmaxf(a, 0.0f));
}
__device__ __forceinline__ float pg_inverse(const PgDev& t, float D) {
    if (t.inverse != 2) {                    // tf_inverse_float kind 1 without norm; cg2 = (3/8 or 1/8) gain^2
        const float h = fmaxf(D, 0.0f) * t.gain / 2.0f;
        const float u = (h * h - t.cg2) - t.rn2;
        return t.off + u / t.gain;
    }
    // closed-form approximation of the exact unbiased inverse (Makitalo & Foi): the Poisson inverse, defined from
    // d0 = 2 sqrt(3/8) (the transform of zero photons) upwards, minus s2; below d0 the 1/d^3 term would take over
    const float d = fmaxf(D, t.d0);
    const float d2 = d * d, d3 = d2 * d;
    float y = d2 * 0.25f;
    y = y + t.k1 / d;
    y = y - t.k2 / d2;
    y = y + t.k3 / d3;
    y = y - 0.125f;
    y = y - t.s2;
    return t.off + t.gain * fmaxf(y, 0.0f);
}

constexpr int EW_THREADS = 256;
constexpr int EW_MAX_BLOCKS = 256 * 8;

// ---- 8 voxels per lane: 16-byte uint16 accesses, 2 x 16-byte fp32 accesses ----------------------
__device__ __forceinline__ void ld8(const uint16_t* p, float (&v)[8]) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        v[2 * i] = (float)(w[i] & 0xFFFFu);
        v[2 * i + 1] = (float)(w[i] >> 16);
    }
}
__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void st8(uint16_t* p, const uint16_t (&q)[8]) {
    uint4 r;
    r.x = (unsigned)q[0] | ((unsigned)q[1] << 16);
    r.y = (unsigned)q[2] | ((unsigned)q[3] << 16);
    r.z = (unsigned)q[4] | ((unsigned)q[5] << 16);
    r.w = (unsigned)q[6] | ((unsigned)q[7] << 16);
    *reinterpret_cast<uint4*>(p) = r;
}

// A stream operator provides one(i) for a single voxel and eight(i) for voxels [i, i+8).
template <class Op>
__global__ __launch_bounds__(EW_THREADS) void stream8_kernel(Op op, size_t n8) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n8; g += stride)
        op.eight(8 * g);
}
template <class Op>
__global__ __launch_bounds__(EW_THREADS) void stream1_kernel(Op op, size_t begin, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = begin + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        op.one(i);
}

struct OpCountsFromU16 {
    const uint16_t* in;
    float* out;
    float offset;
    __device__ void one(size_t i) const { out[i] = (float)in[i] - offset; }
    __device__ void eight(size_t i) const {
        float v[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = v[k] - offset;
        st8(out + i, v);
    }
};
// the same, plus the counts XOR 0x8000 (= v - 32768 as int16) for the integer block matching
struct OpCountsFromU16Both {
    const uint16_t* in;
    float* out;
    uint16_t* out16;
    float offset;
    __device__ void one(size_t i) const {
        out[i] = (float)in[i] - offset;
        out16[i] = (uint16_t)(in[i] ^ 0x8000u);
    }
    __device__ void eight(size_t i) const {
        const uint4 r = *reinterpret_cast<const uint4*>(in + i);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (float)(w[k] & 0xFFFFu) - offset;
            v[2 * k + 1] = (float)(w[k] >> 16) - offset;
        }
        st8(out + i, v);
        *reinterpret_cast<uint4*>(out16 + i) =
            make_uint4(r.x ^ 0x80008000u, r.y ^ 0x80008000u, r.z ^ 0x80008000u, r.w ^ 0x80008000u);
    }
};
struct OpNormalizeU16 {
    const float* num;
    const float* den;
    uint16_t* out;
    float offset;
    __device__ void one(size_t i) const { out[i] = quantise_u16(num[i] / den[i] + offset, 65535.0f); }
    __device__ void eight(size_t i) const {
        float a[8], b[8];
        uint16_t q[8];
        ld8(num + i, a);
        ld8(den + i, b);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = quantise_u16(a[k] / b[k] + offset, 65535.0f);
        st8(out + i, q);
    }
};
// what stage 2 of the uint16 pipelines matches on -- the basic estimate as the counts a uint16
// caller would see.  As fp32 (counts - offset: the float kernel's input) or as counts XOR 0x8000 (the integer
// kernel's); the Wiener filter itself keeps the unrounded estimate.
struct OpRoundCountsF32 {
    const float* in;
    float* out;
    float offset;
    __device__ void one(size_t i) const { out[i] = (float)quantise_u16(in[i] + offset, 65535.0f) - offset; }
    __device__ void eight(size_t i) const {
        float v[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (float)quantise_u16(v[k] + offset, 65535.0f) - offset;
        st8(out + i, v);
    }
};
struct OpRoundCountsU16 {
    const float* in;
    uint16_t* out16;
    float offset;
    __device__ void one(size_t i) const {
        out16[i] = (uint16_t)(quantise_u16(in[i] + offset, 65535.0f) ^ 0x8000u);
    }
    __device__ void eight(size_t i) const {
        float v[8];
        uint16_t q[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = (uint16_t)(quantise_u16(v[k] + offset, 65535.0f) ^ 0x8000u);
        st8(out16 + i, q);
    }
};
template <typename TIn>
struct OpTfForward {
    TfDev t;
    const TIn* in;
    float* out;
    __device__ void one(size_t i) const { out[i] = tf_forward(t, (float)in[i]); }
    __device__ void eight(size_t i) const {
        float v[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = tf_forward(t, v[k]);
        st8(out + i, v);
    }
};
struct OpTfInverseU16 {
    TfDev t;
    const float* in;
    uint16_t* out;
    __device__ void one(size_t i) const { out[i] = quantise_u16(tf_inverse_float(t, in[i]), t.maxc); }
    __device__ void eight(size_t i) const {
        float v[8];
        uint16_t q[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = quantise_u16(tf_inverse_float(t, v[k]), t.maxc);
        st8(out + i, q);
    }
};
struct OpPgForwardU16 {
    PgDev t;
    const uint16_t* in;
    float* out;
    __device__ void one(size_t i) const { out[i] = pg_forward(t, (float)in[i]); }
    __device__ void eight(size_t i) const {
        float v[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = pg_forward(t, v[k]);
        st8(out + i, v);
    }
};
struct OpPgInverseU16 {
    PgDev t;
    const float* in;
    uint16_t* out;
    __device__ void one(size_t i) const { out[i] = quantise_u16(pg_inverse(t, in[i]), 65535.0f); }
    __device__ void eight(size_t i) const {
        float v[8];
        uint16_t q[8];
        ld8(in + i, v);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = quantise_u16(pg_inverse(t, v[k]), 65535.0f);
        st8(out + i, q);
    }
};
// what an accumulated prediction `a` of weight `w` becomes (OpTileFinalize, tile_stitch_u16_kernel)
__device__ __forceinline__ uint16_t tile_finalize_value(const TfDev& t, float a, float w) {
    const float y = a / (w + 1e-8f);         // accum_wgt += 1e-8 ; accum_pred /= accum_wgt
    return quantise_u16(tf_inverse_float(t, y), t.maxc);
}
struct OpTileFinalize {
    TfDev t;
    const float* acc;
    const float* wgt;
    uint16_t* out;
    __device__ uint16_t f(float a, float w) const { return tile_finalize_value(t, a, w); }
    __device__ void one(size_t i) const { out[i] = f(acc[i], wgt[i]); }
    __device__ void eight(size_t i) const {
        float a[8], w[8];
        uint16_t q[8];
        ld8(acc + i, a);
        ld8(wgt + i, w);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = f(a[k], w[k]);
        st8(out + i, q);
    }
};

// uint16 input has only 65536 distinct values: for the fp64-math-bound asinh transform the
// forward pass becomes a table lookup.  The table is filled by the same device function, so the
// results are bit-identical to direct evaluation.
__global__ __launch_bounds__(EW_THREADS) void tf_lut_build_kernel(TfDev t, float* __restrict__ lut) {
    const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < 65536u) lut[v] = tf_forward(t, (float)v);
}
struct OpLutForward {
    const float* lut;
    const uint16_t* in;
    float* out;
    __device__ void one(size_t i) const { out[i] = lut[in[i]]; }
    __device__ void eight(size_t i) const {
        const uint4 r = *reinterpret_cast<const uint4*>(in + i);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = lut[w[k] & 0xFFFFu];
            v[2 * k + 1] = lut[w[k] >> 16];
        }
        st8(out + i, v);
    }
};

// dst[i] = src[i] != 0: a uint16 mask window (non-zero = foreground) as the bytes a mask pool takes
struct OpNonzeroU8 {
    const uint16_t* in;
    uint8_t* out;
    __device__ void one(size_t i) const { out[i] = in[i] ? 1 : 0; }
    __device__ void eight(size_t i) const {
        const uint4 r = *reinterpret_cast<const uint4*>(in + i);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
        uint2 q;
        q.x = ((w[0] & 0xFFFFu) ? 1u : 0u) | ((w[0] >> 16) ? 1u << 8 : 0u) | ((w[1] & 0xFFFFu) ? 1u << 16 : 0u) |
              ((w[1] >> 16) ? 1u << 24 : 0u);
        q.y = ((w[2] & 0xFFFFu) ? 1u : 0u) | ((w[2] >> 16) ? 1u << 8 : 0u) | ((w[3] & 0xFFFFu) ? 1u << 16 : 0u) |
              ((w[3] >> 16) ? 1u << 24 : 0u);
        *reinterpret_cast<uint2*>(out + i) = q;
    }
};

static inline unsigned ew_blocks(size_t n);
static inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}
// Launch `op` over n voxels: 8 per lane where every pointer is 16-byte aligned, one per lane for
// the tail (or for everything when a caller hands in an unaligned view).
template <class Op>
static hipError_t launch_stream(const Op& op, size_t n, bool vec_ok, hipStream_t s) {
    const size_t n8 = vec_ok ? n / 8 : 0;
    if (n8) hipLaunchKernelGGL(stream8_kernel<Op>, dim3(ew_blocks(n8)), dim3(EW_THREADS), 0, s, op, n8);
    if (8 * n8 < n)
        hipLaunchKernelGGL(stream1_kernel<Op>, dim3(ew_blocks(n - 8 * n8)), dim3(EW_THREADS), 0, s, op,
                           8 * n8, n);
    return hipGetLastError();
}

__global__ __launch_bounds__(EW_THREADS) void normalize_kernel(const float* __restrict__ num,
                                                               const float* __restrict__ den,
                                                               float* __restrict__ out, size_t n,
                                                               float lo, float hi, int do_clip) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float v = num[i] / den[i];
        if (do_clip) v = fminf(fmaxf(v, lo), hi);
        out[i] = v;
    }
}




__global__ __launch_bounds__(EW_THREADS) void tf_inverse_float_kernel(TfDev t,
                                                                      const float* __restrict__ in,
                                                                      float* __restrict__ out,
                                                                      size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = tf_inverse_float(t, in[i]);
}

// ---- overlap tiling ------------------------------------------------------------------------------
struct PatchStarts {
    int v[64 * 3];  // (z,y,x) of up to 64 patches, by value in the kernarg segment
};

__global__ __launch_bounds__(EW_THREADS) void tile_gather_kernel(const float* __restrict__ vol,
                                                                 int nz, int ny, int nx,
                                                                 PatchStarts st, int patch,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.y;
    const int sz0 = st.v[3 * b], sy0 = st.v[3 * b + 1], sx0 = st.v[3 * b + 2];
    const size_t pv = (size_t)patch * patch * patch;
    float* __restrict__ o = out + (size_t)b * pv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pv;
         i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % patch), y = (int)((i / patch) % patch),
                  z = (int)(i / ((size_t)patch * patch));
        const int gz = sz0 + z, gy = sy0 + y, gx = sx0 + x;
        float v = 0.0f;  // add_padding: zeros beyond the volume
        if (gz < nz && gy < ny && gx < nx) v = vol[((size_t)gz * ny + gy) * nx + gx];
        o[i] = v;
    }
}

// One patch per launch: patches of one batch overlap, and the reference adds them one after the
// other in patch order (inference.py:89-103).  Stream order reproduces exactly that order, so the
// sums are bit-identical to the reference's and no atomics are needed.
__global__ __launch_bounds__(EW_THREADS) void tile_accumulate_kernel(const float* __restrict__ pred,
                                                                     int sz0, int sy0, int sx0,
                                                                     int patch, int trim,
                                                                     float* __restrict__ acc,
                                                                     float* __restrict__ wgt,
                                                                     int nz, int ny, int nx) {
    const int core = patch - 2 * trim;
    const size_t cv = (size_t)core * core * core;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cv;
         i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % core), y = (int)((i / core) % core),
                  z = (int)(i / ((size_t)core * core));
        const int gz = sz0 + trim + z, gy = sy0 + trim + y, gx = sx0 + trim + x;
        if (gz < nz && gy < ny && gx < nx) {
            const size_t o = ((size_t)gz * ny + gy) * nx + gx;
            const float p = pred[((size_t)(z + trim) * patch + (y + trim)) * patch + (x + trim)];
            acc[o] = acc[o] + p;
            wgt[o] = wgt[o] + 1.0f;
        }
    }
}

// ---- overlap tiling of one brick of a stored volume ------------------------------
// The brick's patches are a regular grid (TileGrid): patch (iz, iy, ix) starts at index * stride, its linear index
// is raster order over the grid's counts.  One lane per output element, x fastest.
//
// Patches [k0, k0 + nb) of the grid, cut from the uint16 window `win` (origin w0, extent wd, inside a volume of
// `vol`): tf_forward of the count inside the volume, 0.0f beyond it (add_padding pads the transformed image).
// The entry has checked that the window holds every voxel of the grid's patches that lies inside the volume.
__global__ __launch_bounds__(EW_THREADS) void tile_gather_u16_kernel(const uint16_t* __restrict__ win, Int3 w0,
                                                                     Int3 wd, Int3 vol, TfDev t, TileGrid g,
                                                                     long long k0, size_t total,
                                                                     float* __restrict__ out) {
    const size_t pv = (size_t)g.patch * g.patch * g.patch;
    const size_t plane = (size_t)g.count[1] * g.count[2];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t k = (size_t)k0 + i / pv;
        const unsigned r = (unsigned)(i % pv), pe = (unsigned)g.patch;       // patch <= 1024: r < 2^30
        const int x = (int)(r % pe), y = (int)((r / pe) % pe), z = (int)(r / (pe * pe));
        const int gz = (g.first[0] + (int)(k / plane)) * g.stride + z;
        const int gy = (g.first[1] + (int)((k % plane) / g.count[2])) * g.stride + y;
        const int gx = (g.first[2] + (int)(k % g.count[2])) * g.stride + x;
        float v = 0.0f;
        if (gz < vol.v[0] && gy < vol.v[1] && gx < vol.v[2]) {
            const size_t o = ((size_t)(gz - w0.v[0]) * wd.v[1] + (size_t)(gy - w0.v[1])) * wd.v[2] +
                             (size_t)(gx - w0.v[2]);
            v = tf_forward(t, (float)win[o]);
        }
        out[i] = v;
    }
}

// Every voxel of the output box [o0, o0 + oe): the predictions of the grid's patches whose cores hold it, added
// z outermost in increasing patch index -- the order tile_accumulate_kernel's launches give -- then
// tile_finalize_value.  preds: (count_z * count_y * count_x, patch^3) in the grid's raster order.
__global__ __launch_bounds__(EW_THREADS) void tile_stitch_u16_kernel(const float* __restrict__ preds, TileGrid g,
                                                                     int trim, Int3 o0, Int3 oe, TfDev t,
                                                                     uint16_t* __restrict__ out) {
    const int core = g.patch - 2 * trim;
    const size_t pv = (size_t)g.patch * g.patch * g.patch;
    const size_t total = (size_t)oe.v[0] * oe.v[1] * oe.v[2];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int p[3] = {o0.v[0] + (int)(i / ((size_t)oe.v[1] * oe.v[2])), o0.v[1] + (int)((i / oe.v[2]) % oe.v[1]),
                          o0.v[2] + (int)(i % oe.v[2])};
        int lo[3], hi[3];                    // patch indices i with i * stride + trim <= p < i * stride + trim + core
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int d = p[a] - trim, u = d - core + 1;
            lo[a] = u <= 0 ? 0 : (u + g.stride - 1) / g.stride;
            hi[a] = d < 0 ? -1 : d / g.stride;
            lo[a] = lo[a] > g.first[a] ? lo[a] : g.first[a];
            hi[a] = hi[a] < g.first[a] + g.count[a] - 1 ? hi[a] : g.first[a] + g.count[a] - 1;
        }
        float s = 0.0f, w = 0.0f;
        for (int iz = lo[0]; iz <= hi[0]; iz++)
            for (int iy = lo[1]; iy <= hi[1]; iy++)
                for (int ix = lo[2]; ix <= hi[2]; ix++) {
                    const size_t k = ((size_t)(iz - g.first[0]) * g.count[1] + (size_t)(iy - g.first[1])) *
                                         g.count[2] + (size_t)(ix - g.first[2]);
                    const size_t r = ((size_t)(p[0] - iz * g.stride) * g.patch + (size_t)(p[1] - iy * g.stride)) *
                                         g.patch + (size_t)(p[2] - ix * g.stride);
                    s = s + preds[k * pv + r];
                    w = w + 1.0f;
                }
        out[i] = tile_finalize_value(t, s, w);
    }
}


// ---- chunked byte-plane histograms (row f-1) -----------------------------------------------------
// One workgroup per chunk; LDS integer atomics (full rate, unlike ds_add_f32) on 2 x 256 bins.
__global__ __launch_bounds__(EW_THREADS) void chunk_hist_kernel(const uint16_t* __restrict__ vol,
                                                                int nz, int ny, int nx, int cz,
                                                                int cy, int cx, int gcy, int gcx,
                                                                uint32_t* __restrict__ hist) {
    __shared__ unsigned int h[512];
    for (int i = threadIdx.x; i < 512; i += EW_THREADS) h[i] = 0u;
    __syncthreads();
    const int c = blockIdx.x;
    const int bx = c % gcx, by = (c / gcx) % gcy, bz = c / (gcx * gcy);
    const int z0 = bz * cz, y0 = by * cy, x0 = bx * cx;
    const int ez = min(cz, nz - z0), ey = min(cy, ny - y0), ex = min(cx, nx - x0);
    const size_t total = (size_t)ez * ey * ex;
    for (size_t i = threadIdx.x; i < total; i += EW_THREADS) {
        const int x = (int)(i % ex), y = (int)((i / ex) % ey), z = (int)(i / ((size_t)ex * ey));
        const unsigned v = vol[((size_t)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x)];
        atomicAdd(&h[v & 255u], 1u);
        atomicAdd(&h[256u + (v >> 8)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += EW_THREADS) hist[(size_t)c * 512 + i] = h[i];
}

hipError_t launch_chunk_hist(const uint16_t* vol, int nz, int ny, int nx, int cz, int cy, int cx,
                             uint32_t* hist, hipStream_t s) {
    const int gz = (nz + cz - 1) / cz, gy = (ny + cy - 1) / cy, gx = (nx + cx - 1) / cx;
    hipLaunchKernelGGL(chunk_hist_kernel, dim3((unsigned)(gz * gy * gx)), dim3(EW_THREADS), 0, s,
                       vol, nz, ny, nx, cz, cy, cx, gy, gx, hist);
    return hipGetLastError();
}

// ---- counts <-> the pipelines' fp32 values ----------------------------------------------------------------------
// The uint16 pipelines work on counts - offset and write quantise(estimate + offset); under Poisson-Gaussian noise
//  on the stabilised D = pg_forward(count), and write quantise(pg_inverse(estimate)).  The chunk
// kernels and the fused normalisation below take either as their `Epi`.
struct EpiOffset { float offset; };
struct EpiPg { PgDev t; };
__device__ __forceinline__ float epi_f32(const EpiOffset& e, unsigned v) { return (float)v - e.offset; }
__device__ __forceinline__ float epi_f32(const EpiPg& e, unsigned v) { return pg_forward(e.t, (float)v); }
__device__ __forceinline__ uint16_t epi_u16(const EpiOffset& e, float r) {
    return quantise_u16(r + e.offset, 65535.0f);
}
__device__ __forceinline__ uint16_t epi_u16(const EpiPg& e, float r) {
    return quantise_u16(pg_inverse(e.t, r), 65535.0f);
}

// ---- chunk-local mode (BASELINE config 4) ------------------------------
// A batch of padded chunks: chunk (bz, by, bx) of a sub-grid has its core at (z0 + bz*cz, ...),
// extent (ez, ey, ex), and is read with (lz, ly, lx) voxels in front and (pz - ez - lz, ...) behind
// it -- the halo, cut off where the buffer ends.  gather: u16 -> epi_f32 into [batch][pz][py][px] (out16: also the
// counts XOR 0x8000); scatter: the denoised padded chunks' cores -> epi_u16 into the output.
// Element i of a batch of (ez, ey, ex) boxes, one box per chunk: batch entry b, the place (z, y, x) in its box, and
// the buffer coordinates (cz0, cy0, cx0) of that chunk's core.
struct ChunkVoxel { int b, z, y, x, cz0, cy0, cx0; };
__device__ __forceinline__ ChunkVoxel chunk_voxel(const ChunkBatch& cb, size_t i, int ez, int ey, int ex) {
    const size_t vox = (size_t)ez * ey * ex;
    ChunkVoxel v;
    v.b = (int)(i / vox);
    const size_t r = i - (size_t)v.b * vox;
    v.x = (int)(r % ex); v.y = (int)((r / ex) % ey); v.z = (int)(r / ((size_t)ex * ey));
    const int c = cb.first + v.b;
    const int bx = c % cb.sgx, by = (c / cb.sgx) % cb.sgy, bz = c / (cb.sgx * cb.sgy);
    v.cz0 = cb.z0 + bz * cb.cz; v.cy0 = cb.y0 + by * cb.cy; v.cx0 = cb.x0 + bx * cb.cx;
    return v;
}
template <class Epi>
__global__ __launch_bounds__(EW_THREADS) void chunk_gather_kernel(const uint16_t* __restrict__ in, ChunkBatch cb,
                                                                  Epi epi, float* __restrict__ out,
                                                                  uint16_t* __restrict__ out16) {
    const size_t total = (size_t)cb.pz * cb.py * cb.px * (size_t)cb.count;
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total;
         i += (size_t)gridDim.x * EW_THREADS) {
        const ChunkVoxel p = chunk_voxel(cb, i, cb.pz, cb.py, cb.px);
        const int gz = min(max(p.cz0 - cb.lz + p.z, 0), cb.nz - 1);
        const int gy = min(max(p.cy0 - cb.ly + p.y, 0), cb.ny - 1);
        const int gx = min(max(p.cx0 - cb.lx + p.x, 0), cb.nx - 1);
        const unsigned v = in[((size_t)gz * cb.ny + gy) * cb.nx + gx];
        out[i] = epi_f32(epi, v);
        if (out16) out16[i] = (uint16_t)(v ^ 0x8000u);
    }
}
template <class Epi>
__global__ __launch_bounds__(EW_THREADS) void chunk_scatter_kernel(const float* __restrict__ est, ChunkBatch cb,
                                                                   Epi epi, uint16_t* __restrict__ out) {
    const size_t total = (size_t)cb.ez * cb.ey * cb.ex * (size_t)cb.count;
    const size_t pvox = (size_t)cb.pz * cb.py * cb.px;
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total;
         i += (size_t)gridDim.x * EW_THREADS) {
        const ChunkVoxel p = chunk_voxel(cb, i, cb.ez, cb.ey, cb.ex);
        const float v =
            est[(size_t)p.b * pvox + ((size_t)(p.z + cb.lz) * cb.py + (p.y + cb.ly)) * cb.px + (p.x + cb.lx)];
        const int oz = p.cz0 + p.z - cb.out_z0, oy = p.cy0 + p.y, ox = p.cx0 + p.x;
        out[((size_t)oz * cb.ny + oy) * cb.nx + ox] = epi_u16(epi, v);
    }
}
static unsigned chunk_blocks(size_t total) {
    return (unsigned)std::min<size_t>((total + EW_THREADS - 1) / EW_THREADS, 1u << 20);
}
hipError_t launch_chunk_gather(const uint16_t* in, const ChunkBatch& cb, const ChunkMap& m, float* out,
                               hipStream_t s, uint16_t* out16) {
    const dim3 grid(chunk_blocks((size_t)cb.pz * cb.py * cb.px * (size_t)cb.count));
    if (m.pg)
        hipLaunchKernelGGL(chunk_gather_kernel<EpiPg>, grid, dim3(EW_THREADS), 0, s, in, cb, EpiPg{*m.pg}, out, out16);
    else
        hipLaunchKernelGGL(chunk_gather_kernel<EpiOffset>, grid, dim3(EW_THREADS), 0, s, in, cb, EpiOffset{m.offset},
                           out, out16);
    return hipGetLastError();
}
hipError_t launch_chunk_scatter(const float* est, const ChunkBatch& cb, const ChunkMap& m, uint16_t* out,
                                hipStream_t s) {
    const dim3 grid(chunk_blocks((size_t)cb.ez * cb.ey * cb.ex * (size_t)cb.count));
    if (m.pg)
        hipLaunchKernelGGL(chunk_scatter_kernel<EpiPg>, grid, dim3(EW_THREADS), 0, s, est, cb, EpiPg{*m.pg}, out);
    else
        hipLaunchKernelGGL(chunk_scatter_kernel<EpiOffset>, grid, dim3(EW_THREADS), 0, s, est, cb, EpiOffset{m.offset},
                           out);
    return hipGetLastError();
}

// ---- denominator of the aggregation as a convolution (stage_kernels.hip) -------------------------
// The stage kernels leave sum(rint(u 2^40)) of the blocks on their corner voxels (64-bit integers, exact
// whatever the order of the atomics).  C = fl32(cw 2^-40); out(i) = sum_{t=0..7} k[t] * in(i - t) along
// one axis: a block corner c with weight u spreads u * k[t] over voxels c .. c + 7.  Fixed summation
// order (fmaf chain, t ascending, from +0): DESIGN.md 3.8, oracle orc_den_from_corners.
struct Win1D {
    float k[8];
};
__device__ __forceinline__ float cw_to_float(unsigned long long c) {
    // c < 2^53 (at most 2^12 blocks of at most 2^40 per corner): both conversions and the scaling are
    // exact, the cast to float rounds once
    return (float)(((double)(unsigned)(c >> 32) * 4294967296.0 + (double)(unsigned)c) * 9.094947017729282e-13);
}
// int64 fixed point -> fp32: fl64(num) (one rounding beyond 2^53), exact scaling, one rounding to fp32
__device__ __forceinline__ float num_to_float(long long v, double down) {
    return (float)(__ll2double_rn(v) * down);
}
// along y or z: one thread per line (lanes along x: coalesced), marching with the last 8 inputs
// in registers, so every input is read once.  Line (o, i): base = o * extent * inner + i,
// element stride `inner`.
// With XFIRST the input is the corner-weight volume and the value fed into the line is the 8-tap
// convolution along x of its row (8 neighbouring loads, L1 hits), which fuses the x and y passes.
template <bool XFIRST>
__global__ __launch_bounds__(EW_THREADS) void conv8_line_kernel(const void* __restrict__ in_,
                                                                float* __restrict__ out, size_t nlines,
                                                                size_t inner, int extent, Win1D w) {
    for (size_t l = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; l < nlines;
         l += (size_t)gridDim.x * EW_THREADS) {
        const size_t o = l / inner, i = l - o * inner;
        const size_t base = o * (size_t)extent * inner + i;
        float h[8];
#pragma unroll
        for (int t = 0; t < 8; t++) h[t] = 0.0f;
        for (int e = 0; e < extent; e++) {
#pragma unroll
            for (int t = 7; t > 0; t--) h[t] = h[t - 1];
            if (XFIRST) {
                // lines run along y, `inner` is the row length and i the x coordinate
                const unsigned long long* row = static_cast<const unsigned long long*>(in_) + base + (size_t)e * inner;
                float ax = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; t++)
                    if ((size_t)t <= i) ax = fmaf(w.k[t], cw_to_float(*(row - t)), ax);
                h[0] = ax;
            } else {
                h[0] = static_cast<const float*>(in_)[base + (size_t)e * inner];
            }
            float acc = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; t++) acc = fmaf(w.k[t], h[t], acc);
            out[base + (size_t)e * inner] = acc;
        }
    }
}

// Fused x / y pass for row lengths that are multiples of 4: one thread owns four consecutive x
// outputs and marches along y.  Per row it loads its own four corner weights and the eight to its left
// (six 16-byte loads for four outputs), forms the four x-convolutions in registers and pushes them
// through four 8-deep y shift registers.
__global__ __launch_bounds__(EW_THREADS) void conv8_xy4_kernel(const unsigned long long* __restrict__ in,
                                                               float* __restrict__ out, size_t nlines,
                                                               int nx4, int ny, Win1D w) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    for (size_t l = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; l < nlines;
         l += (size_t)gridDim.x * EW_THREADS) {
        const size_t o = l / (size_t)nx4;              // (volume, z) index
        const int x0 = 4 * (int)(l - o * (size_t)nx4);
        const size_t nx = 4 * (size_t)nx4;
        const size_t base = o * (size_t)ny * nx + (size_t)x0;
        float h[8][4];
#pragma unroll
        for (int t = 0; t < 8; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) h[t][j] = 0.0f;
        for (int y = 0; y < ny; y++) {
            const unsigned long long* row = in + base + (size_t)y * nx;
            float win_[12];
#pragma unroll
            for (int q = 0; q < 6; q++) {
                // elements row[2 q - 8], row[2 q - 7]: left of the row start they count as zero
                u64x2 v = {0ull, 0ull};
                if (x0 + 2 * q - 8 >= 0) v = *reinterpret_cast<const u64x2*>(row + 2 * q - 8);
                win_[2 * q] = cw_to_float(v.x);
                win_[2 * q + 1] = cw_to_float(v.y);
            }
#pragma unroll
            for (int t = 7; t > 0; t--)
#pragma unroll
                for (int j = 0; j < 4; j++) h[t][j] = h[t - 1][j];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float ax = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; t++) ax = fmaf(w.k[t], win_[8 + j - t], ax);
                h[0][j] = ax;
            }
            float r[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float acc = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; t++) acc = fmaf(w.k[t], h[t][j], acc);
                r[j] = acc;
            }
            *reinterpret_cast<float4*>(out + base + (size_t)y * nx) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

// The z pass of the denominator convolution fused into the normalisation (round 3): a thread owns W
// consecutive x of one (volume, y) line and marches along z with the 8-deep shift register of
// conv8_line_kernel -- den = the same fmaf chain, in the same order -- then
// out = fl32(fl64(num) 2^(E - 43)) / den (+ clip, or + offset, clamp, rint, uint16).  Saves the pass that
// would write den and the one that would read it back; bit-identical to the separate passes of the staged
// entry points.
// The uint16 form's last step on the quotient r is the Epi's epi_u16 (under EpiPg the estimate never travels to
// HBM as fp32).
template <int W, bool U16, class Epi>
__global__ __launch_bounds__(EW_THREADS) void normalize_zconv_kernel(const long long* __restrict__ num,
                                                                     const double* __restrict__ qscale,
                                                                     const float* __restrict__ txy,
                                                                     void* __restrict__ out, size_t nlines,
                                                                     size_t plane, int nz, Win1D w, float lo,
                                                                     float hi, int do_clip, Epi epi,
                                                                     const float* __restrict__ pair_src,
                                                                     float* __restrict__ pair_out,
                                                                     uint16_t* __restrict__ match16,
                                                                     float match_offset) {
    // epi: what the uint16 form does to the quotient.  In front of the by-products on purpose: as the last argument
    // it costs the wide uint16 instance 70 VGPRs instead of 56, one wave per SIMD less
    // pair_out (fp32 output, W = 4 only): additionally the interleaved volume (pair_src, out) the Wiener
    // kernel gathers from, so that it does not cost a pass of its own
    // match16 (fp32 output): additionally the estimate rounded to counts, XOR 0x8000 -- what stage 2 of the
    // uint16 pipelines matches on in the integer kernel (OpRoundCountsU16 as a pass: 2.5 ms)
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const size_t lines_per_vol = plane / W;
    for (size_t l = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; l < nlines;
         l += (size_t)gridDim.x * EW_THREADS) {
        const size_t o = l / lines_per_vol, i = l - o * lines_per_vol;
        const size_t base = o * (size_t)nz * plane + (size_t)W * i;
        const double down = qscale[2 * o + 1];
        float h[8][W];
#pragma unroll
        for (int t = 0; t < 8; t++)
#pragma unroll
            for (int j = 0; j < W; j++) h[t][j] = 0.0f;
        for (int z = 0; z < nz; z++) {
            const size_t at = base + (size_t)z * plane;
#pragma unroll
            for (int t = 7; t > 0; t--)
#pragma unroll
                for (int j = 0; j < W; j++) h[t][j] = h[t - 1][j];
            float a[W];
            if (W == 4) {
                const float4 c = *reinterpret_cast<const float4*>(txy + at);
                const i64x2 m0 = *reinterpret_cast<const i64x2*>(num + at);
                const i64x2 m1 = *reinterpret_cast<const i64x2*>(num + at + 2);
                h[0][0] = c.x; h[0][1 % W] = c.y; h[0][2 % W] = c.z; h[0][3 % W] = c.w;
                a[0] = num_to_float(m0.x, down); a[1 % W] = num_to_float(m0.y, down);
                a[2 % W] = num_to_float(m1.x, down); a[3 % W] = num_to_float(m1.y, down);
            } else {
                h[0][0] = txy[at];
                a[0] = num_to_float(num[at], down);
            }
            float r[W];
#pragma unroll
            for (int j = 0; j < W; j++) {
                float den = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; t++) den = fmaf(w.k[t], h[t][j], den);
                r[j] = a[j] / den;
            }
            if (U16) {
                uint16_t* o16 = static_cast<uint16_t*>(out) + at;
                if (W == 4) {
                    const uint32_t q0 = epi_u16(epi, r[0]), q1 = epi_u16(epi, r[1 % W]);
                    const uint32_t q2 = epi_u16(epi, r[2 % W]), q3 = epi_u16(epi, r[3 % W]);
                    *reinterpret_cast<uint2*>(o16) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
                } else {
                    o16[0] = epi_u16(epi, r[0]);
                }
            } else {
                float* o32 = static_cast<float*>(out) + at;
#pragma unroll
                for (int j = 0; j < W; j++)
                    if (do_clip) r[j] = fminf(fmaxf(r[j], lo), hi);
                if (match16) {
                    uint16_t* m16 = match16 + at;
                    if (W == 4) {
                        const uint32_t q0 = quantise_u16(r[0] + match_offset, 65535.0f) ^ 0x8000u;
                        const uint32_t q1 = quantise_u16(r[1 % W] + match_offset, 65535.0f) ^ 0x8000u;
                        const uint32_t q2 = quantise_u16(r[2 % W] + match_offset, 65535.0f) ^ 0x8000u;
                        const uint32_t q3 = quantise_u16(r[3 % W] + match_offset, 65535.0f) ^ 0x8000u;
                        *reinterpret_cast<uint2*>(m16) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
                    } else {
                        m16[0] = (uint16_t)(quantise_u16(r[0] + match_offset, 65535.0f) ^ 0x8000u);
                    }
                }
                if (W == 4) {
                    *reinterpret_cast<float4*>(o32) = make_float4(r[0], r[1 % W], r[2 % W], r[3 % W]);
                    if (pair_out) {
                        const float4 s4 = *reinterpret_cast<const float4*>(pair_src + at);
                        float4* po = reinterpret_cast<float4*>(pair_out + 2 * at);
                        po[0] = make_float4(s4.x, r[0], s4.y, r[1 % W]);
                        po[1] = make_float4(s4.z, r[2 % W], s4.w, r[3 % W]);
                    }
                } else {
                    o32[0] = r[0];
                }
            }
        }
    }
}

static dim3 conv_blocks(size_t items) {
    size_t b = (items + EW_THREADS - 1) / EW_THREADS;
    if (b > 65536) b = 65536;
    return dim3((unsigned)(b ? b : 1));
}
// den's x / y passes only (cw -> tmp); the z pass then rides with the normalisation (launch_normalize_zconv)
hipError_t launch_den_xy_from_corners(const unsigned long long* cw, float* tmp, int nz, int ny, int nx, int batch,
                                      const float* win1d, hipStream_t s) {
    Win1D w;
    for (int t = 0; t < 8; t++) w.k[t] = win1d[t];
    if (nx % 4 == 0 && ((uintptr_t)cw & 15u) == 0 && ((uintptr_t)tmp & 15u) == 0) {
        const size_t lines4 = (size_t)batch * nz * (nx / 4);
        hipLaunchKernelGGL(conv8_xy4_kernel, conv_blocks(lines4), dim3(EW_THREADS), 0, s, cw, tmp, lines4, nx / 4, ny, w);
    } else {
        const size_t ylines = (size_t)batch * nz * nx;
        hipLaunchKernelGGL((conv8_line_kernel<true>), conv_blocks(ylines), dim3(EW_THREADS), 0, s,
                           static_cast<const void*>(cw), tmp, ylines, (size_t)nx, ny, w);
    }
    return hipGetLastError();
}

// out = fl32(fl64(num) 2^(E - 43)) / (txy (*)_z win)
template <int W, bool U16, class Epi>
static void zconv_launch(const NormSums& in, const NormOut& out, hipStream_t s, const NormSide& side, const Epi& epi) {
    Win1D w;
    for (int t = 0; t < 8; t++) w.k[t] = in.win1d[t];
    const size_t plane = (size_t)in.ny * in.nx, nlines = (size_t)in.batch * (plane / W);
    void* dst = U16 ? static_cast<void*>(out.u16) : static_cast<void*>(out.f32);
    hipLaunchKernelGGL((normalize_zconv_kernel<W, U16, Epi>), conv_blocks(nlines), dim3(EW_THREADS), 0, s, in.num,
                       in.qscale, in.txy, dst, nlines, plane, in.nz, w, out.lo, out.hi, out.clip ? 1 : 0, epi,
                       side.pair_src, side.pair_out, side.round16, side.round_offset);
}
NormWrote launch_normalize_zconv(const NormSums& in, const NormOut& out, hipStream_t s, const NormSide* side) {
    if (out.pg && !out.u16) return {hipErrorInvalidValue, false, false};
    const size_t plane = (size_t)in.ny * in.nx;
    const void* dst = out.u16 ? static_cast<const void*>(out.u16) : static_cast<const void*>(out.f32);
    const bool wide = plane % 4 == 0 && ((uintptr_t)in.num & 15u) == 0 && ((uintptr_t)in.txy & 15u) == 0 &&
                      ((uintptr_t)dst & 15u) == 0 && ((size_t)in.nz * plane) % 4 == 0;
    NormSide can{nullptr, nullptr, nullptr, 0.0f};      // the by-products this launch writes
    if (side && out.f32) {
        // the pair volume only in the wide form (16-byte stores), the rounded copy only of the UNCLIPPED estimate
        // (8-byte stores in the wide form)
        if (wide && side->pair_src && side->pair_out && ((uintptr_t)side->pair_src & 15u) == 0 &&
            ((uintptr_t)side->pair_out & 15u) == 0) {
            can.pair_src = side->pair_src;
            can.pair_out = side->pair_out;
        }
        if (!out.clip && ((uintptr_t)side->round16 & 7u) == 0) {
            can.round16 = side->round16;
            can.round_offset = side->round_offset;
        }
    }
    const EpiOffset off{out.offset};
    if (out.pg) {
        const EpiPg pg{*out.pg};
        wide ? zconv_launch<4, true>(in, out, s, can, pg) : zconv_launch<1, true>(in, out, s, can, pg);
    } else if (out.u16) {
        wide ? zconv_launch<4, true>(in, out, s, can, off) : zconv_launch<1, true>(in, out, s, can, off);
    } else {
        wide ? zconv_launch<4, false>(in, out, s, can, off) : zconv_launch<1, false>(in, out, s, can, off);
    }
    return {hipGetLastError(), can.pair_out != nullptr, can.round16 != nullptr};
}

// the staged entry point's form: all three passes, den written
hipError_t launch_den_from_corners(const unsigned long long* cw, float* tmp, float* den, int nz, int ny, int nx,
                                   int batch, const float* win1d, hipStream_t s) {
    hipError_t e = launch_den_xy_from_corners(cw, tmp, nz, ny, nx, batch, win1d, s);
    if (e != hipSuccess) return e;
    Win1D w;
    for (int t = 0; t < 8; t++) w.k[t] = win1d[t];
    const size_t zlines = (size_t)batch * ny * nx;
    hipLaunchKernelGGL((conv8_line_kernel<false>), conv_blocks(zlines), dim3(EW_THREADS), 0, s,
                       static_cast<const void*>(tmp), den, zlines, (size_t)ny * nx, nz, w);
    return hipGetLastError();
}

__global__ __launch_bounds__(EW_THREADS) void num_to_float_kernel(const long long* __restrict__ num,
                                                                  const double* __restrict__ qscale,
                                                                  float* __restrict__ out, size_t nvox) {
    const double down = qscale[2 * blockIdx.y + 1];
    const size_t off = (size_t)blockIdx.y * nvox;
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < nvox; i += (size_t)gridDim.x * EW_THREADS)
        out[off + i] = num_to_float(num[off + i], down);
}
hipError_t launch_num_to_float(const long long* num, const double* qscale, float* out, size_t nvox, int batch,
                               hipStream_t s) {
    size_t b = (nvox + EW_THREADS - 1) / EW_THREADS;
    if (b > 16384) b = 16384;
    hipLaunchKernelGGL(num_to_float_kernel, dim3((unsigned)(b ? b : 1), (unsigned)batch), dim3(EW_THREADS), 0, s, num,
                       qscale, out, nvox);
    return hipGetLastError();
}

// ---- the numerator's unit -----------------------------------------------------------
// E with max |v| < 2^E from the largest |v| bit pattern of each volume (an integer maximum: exact and
// order-independent), then qscale[2 b] = 2^(43 - E), qscale[2 b + 1] = 2^(E - 43).
__global__ __launch_bounds__(EW_THREADS) void absmax_bits_kernel(const float* __restrict__ vol, size_t nvox,
                                                                 unsigned* __restrict__ maxbits) {
    const float* v = vol + (size_t)blockIdx.y * nvox;
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < nvox; i += (size_t)gridDim.x * EW_THREADS)
        m = max(m, __float_as_uint(v[i]) & 0x7FFFFFFFu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxbits + blockIdx.y, m);
}
__global__ void qscale_kernel(const unsigned* __restrict__ maxbits, int batch, int fixed_exp,
                              double* __restrict__ qscale, unsigned* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int E = fixed_exp != INT32_MIN ? fixed_exp : (int)(maxbits[b] >> 23) - 126;
    // DESIGN.md 3.8, domain: beyond |v| < 2^56 the squares of transform coefficients (|Y| <= sqrt(8192) max|v|)
    // and of voxel differences leave fp32; infinities and NaNs land here too.  The pipeline still runs (no
    // fault, garbage out); the host reports EXABM4D_ERR_INVALID at its next synchronisation (status bit 1).
    if (E > 56 && status) __hip_atomic_fetch_or(status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    qscale[2 * b] = ldexp(1.0, 43 - E);
    qscale[2 * b + 1] = ldexp(1.0, E - 43);
}
hipError_t launch_qscale(const float* vol, size_t nvox, int batch, int fixed_exp, unsigned* maxbits,
                         double* qscale, hipStream_t s, unsigned* status) {
    if (fixed_exp == INT32_MIN) {
        hipError_t e = hipMemsetAsync(maxbits, 0, sizeof(unsigned) * (size_t)batch, s);
        if (e != hipSuccess) return e;
        size_t b = (nvox + (size_t)EW_THREADS * 8 - 1) / ((size_t)EW_THREADS * 8);
        if (b > 4096) b = 4096;
        hipLaunchKernelGGL(absmax_bits_kernel, dim3((unsigned)(b ? b : 1), (unsigned)batch), dim3(EW_THREADS), 0, s, vol,
                           nvox, maxbits);
    }
    hipLaunchKernelGGL(qscale_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, maxbits, batch, fixed_exp,
                       qscale, status);
    return hipGetLastError();
}

static inline unsigned ew_blocks(size_t n) {
    size_t b = (n + EW_THREADS - 1) / EW_THREADS;
    if (b > (size_t)EW_MAX_BLOCKS) b = EW_MAX_BLOCKS;
    if (b == 0) b = 1;
    return (unsigned)b;
}

hipError_t launch_normalize(const float* num, const float* den, float* out, size_t n, float lo,
                            float hi, hipStream_t s) {
    hipLaunchKernelGGL(normalize_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, s, num, den, out,
                       n, lo, hi, lo <= hi ? 1 : 0);
    return hipGetLastError();
}
hipError_t launch_counts_from_u16(const uint16_t* in, float* out, size_t n, float offset,
                                  hipStream_t s, uint16_t* out16) {
    if (out16)
        return launch_stream(OpCountsFromU16Both{in, out, out16, offset}, n,
                             aligned16(in, out) && ((uintptr_t)out16 & 15) == 0, s);
    return launch_stream(OpCountsFromU16{in, out, offset}, n, aligned16(in, out), s);
}
hipError_t launch_round_counts(const float* in, float* out_f32, uint16_t* out_u16x, size_t n, float offset,
                               hipStream_t s) {
    if (out_u16x)
        return launch_stream(OpRoundCountsU16{in, out_u16x, offset}, n,
                             aligned16(in, in) && ((uintptr_t)out_u16x & 15) == 0, s);
    return launch_stream(OpRoundCountsF32{in, out_f32, offset}, n, aligned16(in, out_f32), s);
}
hipError_t launch_nonzero_u8(const uint16_t* src, uint8_t* dst, size_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    return launch_stream(OpNonzeroU8{src, dst}, n, ((uintptr_t)src & 15u) == 0 && ((uintptr_t)dst & 7u) == 0, s);
}
hipError_t launch_normalize_u16(const float* num, const float* den, uint16_t* out, size_t n,
                                float offset, hipStream_t s) {
    return launch_stream(OpNormalizeU16{num, den, out, offset}, n, aligned16(num, den, out), s);
}
hipError_t launch_pg_forward_u16(const PgDev& t, const uint16_t* in, float* out, size_t n, hipStream_t s) {
    return launch_stream(OpPgForwardU16{t, in, out}, n, aligned16(in, out), s);
}
hipError_t launch_pg_inverse_u16(const PgDev& t, const float* in, uint16_t* out, size_t n, hipStream_t s) {
    return launch_stream(OpPgInverseU16{t, in, out}, n, aligned16(in, out), s);
}
hipError_t launch_tf_forward_u16(const TfDev& t, const uint16_t* in, float* out, size_t n,
                                 hipStream_t s) {
    return launch_stream(OpTfForward<uint16_t>{t, in, out}, n, aligned16(in, out), s);
}
hipError_t launch_tf_forward_u16_lut(const TfDev& t, float* lut, const uint16_t* in, float* out,
                                     size_t n, hipStream_t s) {
    hipLaunchKernelGGL(tf_lut_build_kernel, dim3(65536 / EW_THREADS), dim3(EW_THREADS), 0, s, t, lut);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_stream(OpLutForward{lut, in, out}, n, aligned16(in, out), s);
}
hipError_t launch_tf_forward_f32(const TfDev& t, const float* in, float* out, size_t n,
                                 hipStream_t s) {
    return launch_stream(OpTfForward<float>{t, in, out}, n, aligned16(in, out), s);
}
hipError_t launch_tf_inverse(const TfDev& t, const float* in, void* out, size_t n, int quant,
                             hipStream_t s) {
    if (quant)
        return launch_stream(OpTfInverseU16{t, in, reinterpret_cast<uint16_t*>(out)}, n,
                             aligned16(in, out), s);
    hipLaunchKernelGGL(tf_inverse_float_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, s, t, in,
                       reinterpret_cast<float*>(out), n);
    return hipGetLastError();
}
hipError_t launch_tile_gather(const float* vol, int nz, int ny, int nx, const int* starts, int nb,
                              int patch, float* out, hipStream_t s) {
    const size_t pv = (size_t)patch * patch * patch;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int cnt = nb - b0 < 64 ? nb - b0 : 64;
        PatchStarts st;
        for (int i = 0; i < 3 * cnt; i++) st.v[i] = starts[3 * b0 + i];
        dim3 grid(ew_blocks(pv) > 64 ? 64 : ew_blocks(pv), (unsigned)cnt);
        hipLaunchKernelGGL(tile_gather_kernel, grid, dim3(EW_THREADS), 0, s, vol, nz, ny, nx, st,
                           patch, out + (size_t)b0 * pv);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t launch_tile_accumulate(const float* preds, const int* starts, int nb, int patch, int trim,
                                  float* acc, float* wgt, int nz, int ny, int nx, hipStream_t s) {
    const size_t pv = (size_t)patch * patch * patch;
    const int core = patch - 2 * trim;
    const size_t cv = (size_t)core * core * core;
    for (int b = 0; b < nb; b++) {
        hipLaunchKernelGGL(tile_accumulate_kernel, dim3(ew_blocks(cv)), dim3(EW_THREADS), 0, s,
                           preds + (size_t)b * pv, starts[3 * b], starts[3 * b + 1],
                           starts[3 * b + 2], patch, trim, acc, wgt, nz, ny, nx);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t launch_tile_finalize(const TfDev& t, const float* acc, const float* wgt, uint16_t* out,
                                size_t n, hipStream_t s) {
    return launch_stream(OpTileFinalize{t, acc, wgt, out}, n, aligned16(acc, wgt, out), s);
}
hipError_t launch_tile_gather_u16(const uint16_t* win, const Int3& w0, const Int3& wd, const Int3& vol,
                                  const TfDev& t, const TileGrid& g, long long k0, int nb, float* out,
                                  hipStream_t s) {
    const size_t total = (size_t)nb * g.patch * g.patch * g.patch;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(tile_gather_u16_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, s, win, w0, wd, vol, t,
                       g, k0, total, out);
    return hipGetLastError();
}
hipError_t launch_tile_stitch_u16(const float* preds, const TileGrid& g, int trim, const Int3& o0, const Int3& oe,
                                  const TfDev& t, uint16_t* out, hipStream_t s) {
    const size_t total = (size_t)oe.v[0] * oe.v[1] * oe.v[2];
    hipLaunchKernelGGL(tile_stitch_u16_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, s, preds, g, trim, o0,
                       oe, t, out);
    return hipGetLastError();
}

}  // namespace exabm4d
