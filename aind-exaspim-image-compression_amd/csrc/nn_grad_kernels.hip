// Backward passes of the BM4DNet stage's NDHWC layers (nn_kernels.hip) and the training loss.
//
// What a training step of the U-Net needs besides the framework's convolutions: the gradients of GroupNorm +
// LeakyReLU, MaxPool3d(2) and trilinear x2 up-sampling on the layout the convolutions use, and the
// foreground-weighted Charbonnier loss (reference machine_learning/losses.py) with its gradient.  The geometry is
// the forward's: x[b][s][c], c fastest, a thread moves four channels, C % 4 == 0 and for the norm
// (C / G) % 4 == 0, 256 % (C / 4) == 0, G <= 32.  No atomics anywhere: every sum is formed by one thread or
// combined in a fixed order from fp64 partials, so every result is a deterministic function of its inputs.
// -ffp-contract=off holds: each fma below is written out.
//
// The three layer gradients are templates on the storage type T of the activations and their gradients (float,
// _Float16, __bf16; Pack<T> of nn_ndhwc.h, as in the forward): a thread's four channels are 16 bytes of fp32 or 8
// of a half type, so grids, chunk plan and combination order are the same for all three.  Loads are widened
// exactly, the arithmetic is the fp32 kernel's expression by expression, and each output element is rounded once
// to T (nearest even; an fp16 overflow becomes +-inf).  So from half inputs dgamma, dbeta and coef are the bits
// the fp32 instance gives on the widened inputs, and dx is that instance's dx rounded once.  gamma, stats, coef,
// dgamma and dbeta are fp32, the partial sums fp64, for every T.  The loss stays fp32 (under autocast the
// network's residual sum is fp32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exabm4d_kernels.h"
#include "nn_ndhwc.h"

namespace exabm4d {

constexpr int NG_THREADS = 256;

// ---- GroupNorm + LeakyReLU backward -----------------------------------------------------------------------
// y = lrelu(z), z = gamma xh + beta, xh = (x - mean) rstd; with dz = dy (y > 0 ? 1 : slope) (the side is taken
// from the forward's OUTPUT, so the two passes cannot disagree about it; slope > 0 makes sign(y) = sign(z)):
//   dbeta[c]  = sum_{b,s} dz            dgamma[c] = sum_{b,s} dz xh
//   dx = rstd (gamma dz - m1 - xh m2),  m1, m2 = the means over a (sample, group) of gamma dz and gamma dz xh
// mean, rstd are the fp32 pair the forward's apply pass used (stats[b][g][2]).
// Pass 1 sums dz and dz xh per (sample, chunk of rows, channel); two small kernels combine them; pass 2 applies.
struct GnGradPlan {
    size_t nchunk, rows_per_chunk;
};
static GnGradPlan gn_grad_plan(int batch, size_t spatial, int C) {
    const int rows_per_iter = NG_THREADS / (C / 4);
    // enough workgroups for the chip (~1024 in all), at least 2 * rows_per_iter rows each, at most 64 per sample
    size_t nchunk = (1024 + (size_t)batch - 1) / (size_t)batch;
    const size_t max_by_rows = spatial / (2 * (size_t)rows_per_iter);
    if (nchunk > max_by_rows) nchunk = max_by_rows;
    if (nchunk > 64) nchunk = 64;
    if (nchunk < 1) nchunk = 1;
    GnGradPlan p;
    p.rows_per_chunk = (spatial + nchunk - 1) / nchunk;
    p.rows_per_chunk = (p.rows_per_chunk + rows_per_iter - 1) / rows_per_iter * rows_per_iter;
    p.nchunk = (spatial + p.rows_per_chunk - 1) / p.rows_per_chunk;
    return p;
}
// workspace: part[batch][nchunk][C][2] and cs[batch][C][2] in fp64, then coef[batch][G][2] = {m1, m2} in fp32
size_t groupnorm_bwd_workspace_bytes(int batch, size_t spatial, int C, int G) {
    const GnGradPlan p = gn_grad_plan(batch, spatial, C);
    const size_t bytes = ((size_t)batch * p.nchunk + (size_t)batch) * (size_t)C * 2 * sizeof(double) +
                         (size_t)batch * G * 2 * sizeof(float);
    return (bytes + 15) & ~(size_t)15;
}

__device__ __forceinline__ float lrelu_grad(float dy, float y, float slope) { return y > 0.0f ? dy : dy * slope; }

template <typename T>
__global__ __launch_bounds__(NG_THREADS) void gn_bwd_partial_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy, size_t spatial, int C,
    int G, int nchunk, size_t rows_per_chunk, const float* __restrict__ stats, float slope,
    double* __restrict__ part) {
    using P = Pack<T>;
    using V = typename P::type;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int lanes = C / 4;                         // four-channel lanes per row; lanes divides NG_THREADS
    const int rows_per_iter = NG_THREADS / lanes;
    const int lane = threadIdx.x % lanes, rsub = threadIdx.x / lanes;
    const size_t r0 = (size_t)chunk * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < spatial ? r0 + rows_per_chunk : spatial;
    const int g = 4 * lane / (C / G);
    const float mean = stats[((size_t)b * G + g) * 2], rstd = stats[((size_t)b * G + g) * 2 + 1];
    const size_t off = (size_t)b * spatial * C;
    const V* x4 = reinterpret_cast<const V*>(x + off) + lane;
    const V* y4 = reinterpret_cast<const V*>(y + off) + lane;
    const V* d4 = reinterpret_cast<const V*>(dy + off) + lane;
    double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};   // the thread's sums: fp64 from the start
    for (size_t r = r0 + rsub; r < r1; r += rows_per_iter) {
        const float4 xv = P::unpack(x4[r * lanes]), yv = P::unpack(y4[r * lanes]), dv = P::unpack(d4[r * lanes]);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
        const float ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float dz = lrelu_grad(ds[j], ys[j], slope);
            const float xh = (xs[j] - mean) * rstd;
            sb[j] += (double)dz;
            sg[j] = fma((double)dz, (double)xh, sg[j]);   // the product of two floats is exact in fp64
        }
    }
    __shared__ double sh[NG_THREADS][8];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        sh[threadIdx.x][2 * j] = sb[j];
        sh[threadIdx.x][2 * j + 1] = sg[j];
    }
    __syncthreads();
    // thread `lane` adds its lane's row slots in a fixed order
    if ((int)threadIdx.x < lanes) {
        double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int rs = 0; rs < rows_per_iter; rs++)
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] += sh[rs * lanes + threadIdx.x][k];
        double* pp = part + (((size_t)b * nchunk + chunk) * C + 4 * threadIdx.x) * 2;
#pragma unroll
        for (int k = 0; k < 8; k++) pp[k] = t[k];
    }
}

// cs[b][c][{0: sum dz, 1: sum dz xh}] over the sample's chunks
__global__ void gn_bwd_chunksum_kernel(const double* __restrict__ part, int batch, int C, int nchunk,
                                       double* __restrict__ cs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * C) return;
    const int b = i / C, c = i - b * C;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nchunk; k++) {
        const double* p = part + (((size_t)b * nchunk + k) * C + c) * 2;
        s += p[0];
        q += p[1];
    }
    cs[(size_t)i * 2] = s;
    cs[(size_t)i * 2 + 1] = q;
}

// threads [0, batch * G): coef[b][g] = {m1, m2};  threads [batch * G, batch * G + C): dgamma[c], dbeta[c]
__global__ void gn_bwd_finish_kernel(const double* __restrict__ cs, int batch, int C, int G, double count,
                                     const float* __restrict__ gamma, float* __restrict__ coef,
                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int cpg = C / G;
    if (i < batch * G) {
        const int b = i / G, g = i - b * G;
        double s1 = 0.0, s2 = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; c++) {
            const double ga = gamma ? (double)gamma[c] : 1.0;
            s1 = fma(ga, cs[((size_t)b * C + c) * 2], s1);
            s2 = fma(ga, cs[((size_t)b * C + c) * 2 + 1], s2);
        }
        coef[(size_t)i * 2] = (float)(s1 / count);
        coef[(size_t)i * 2 + 1] = (float)(s2 / count);
    } else if (i < batch * G + C) {
        const int c = i - batch * G;
        if (!dgamma && !dbeta) return;
        double s = 0.0, q = 0.0;
        for (int b = 0; b < batch; b++) {
            s += cs[((size_t)b * C + c) * 2];
            q += cs[((size_t)b * C + c) * 2 + 1];
        }
        if (dbeta) dbeta[c] = (float)s;
        if (dgamma) dgamma[c] = (float)q;
    }
}

template <typename T>
__global__ __launch_bounds__(NG_THREADS) void gn_bwd_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy, T* __restrict__ dx, size_t spatial,
    int C, int G, const float* __restrict__ gamma, const float* __restrict__ stats, const float* __restrict__ coef,
    float slope) {
    using P = Pack<T>;
    using V = typename P::type;
    const int b = blockIdx.y;
    const int lanes = C / 4;
    const size_t n4 = spatial * (size_t)lanes;
    const size_t off = (size_t)b * spatial * C;
    const V* x4 = reinterpret_cast<const V*>(x + off);
    const V* y4 = reinterpret_cast<const V*>(y + off);
    const V* d4 = reinterpret_cast<const V*>(dy + off);
    V* o4 = reinterpret_cast<V*>(dx + off);
    // NG_THREADS is a multiple of `lanes` (checked by the caller), so is the grid stride: a thread keeps its lane
    const size_t stride = (size_t)gridDim.x * NG_THREADS;
    size_t i = (size_t)blockIdx.x * NG_THREADS + threadIdx.x;
    const int lane = (int)(i % lanes), g = 4 * lane / (C / G);
    float ga[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (gamma)
        for (int j = 0; j < 4; j++) ga[j] = gamma[4 * lane + j];
    const float mean = stats[((size_t)b * G + g) * 2], rstd = stats[((size_t)b * G + g) * 2 + 1];
    const float m1 = coef[((size_t)b * G + g) * 2], m2 = coef[((size_t)b * G + g) * 2 + 1];
    for (; i < n4; i += stride) {
        const float4 xv = P::unpack(x4[i]), yv = P::unpack(y4[i]), dv = P::unpack(d4[i]);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
        const float ds[4] = {dv.x, dv.y, dv.z, dv.w};
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float dz = lrelu_grad(ds[j], ys[j], slope);
            const float xh = (xs[j] - mean) * rstd;
            const float t = fmaf(-xh, m2, ga[j] * dz - m1);
            r[j] = rstd * t;
        }
        o4[i] = P::pack(make_float4(r[0], r[1], r[2], r[3]));
    }
}

template <typename T>
hipError_t launch_groupnorm_lrelu_bwd_ndhwc(const T* x, const T* y, const T* dy, T* dx, int batch, size_t spatial,
                                            int C, int G, const float* gamma, const float* stats, float slope,
                                            float* dgamma, float* dbeta, void* workspace, hipStream_t s) {
    const GnGradPlan p = gn_grad_plan(batch, spatial, C);
    const int lanes = C / 4;
    double* part = static_cast<double*>(workspace);
    double* cs = part + (size_t)batch * p.nchunk * C * 2;
    float* coef = reinterpret_cast<float*>(cs + (size_t)batch * C * 2);
    hipLaunchKernelGGL(gn_bwd_partial_kernel<T>, dim3((unsigned)p.nchunk, (unsigned)batch), dim3(NG_THREADS), 0, s, x, y,
                       dy, spatial, C, G, (int)p.nchunk, p.rows_per_chunk, stats, slope, part);
    const int bc = batch * C;
    hipLaunchKernelGGL(gn_bwd_chunksum_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, s, part, batch, C,
                       (int)p.nchunk, cs);
    const int nf = batch * G + C;
    hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, cs, batch, C, G,
                       (double)spatial * (double)(C / G), gamma, coef, dgamma, dbeta);
    const size_t n4 = spatial * (size_t)lanes;
    size_t blocks = (n4 + NG_THREADS - 1) / NG_THREADS;
    const size_t cap = (8192 + (size_t)batch - 1) / (size_t)batch;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(gn_bwd_apply_kernel<T>, dim3((unsigned)blocks, (unsigned)batch), dim3(NG_THREADS), 0, s, x, y, dy,
                       dx, spatial, C, G, gamma, stats, coef, slope);
    return hipGetLastError();
}

// ---- MaxPool3d(2) backward ----------------------------------------------------------------------------------
// One thread per output window and four channels.  The chosen position is the one torch's max_pool3d records:
// scan in (d, h, w) order, replace the running maximum when v > max or v is NaN -- ties go to the first of the
// equal values (+0 == -0), a window with NaNs to its last NaN.  Stride = kernel: windows do not overlap, the
// thread writes dy there and 0 to the other seven, and the threads of the last windows along an odd extent also
// write 0 to its trailing plane / row / column, so every element of dx is written exactly once.  Half types: the
// comparison runs on the widened values (exact, so the choice is the one among the stored values), and what is
// written is dy's element widened and rounded back, which is that element (a signalling NaN comes back quiet).
template <typename T>
__global__ __launch_bounds__(NG_THREADS) void maxpool2_bwd_ndhwc_kernel(const typename Pack<T>::type* __restrict__ x,
                                                                       const typename Pack<T>::type* __restrict__ dy,
                                                                       typename Pack<T>::type* __restrict__ dx,
                                                                       size_t total, int OD, int OH, int OW, int D,
                                                                       int H, int W, int lanes) {
    using P = Pack<T>;
    for (size_t o = (size_t)blockIdx.x * NG_THREADS + threadIdx.x; o < total; o += (size_t)gridDim.x * NG_THREADS) {
        const int l = (int)(o % lanes);
        size_t t = o / lanes;
        const int ow = (int)(t % OW); t /= OW;
        const int oh = (int)(t % OH); t /= OH;
        const int od = (int)(t % OD);
        const size_t b = t / OD;
        const size_t base = (((b * D + 2 * od) * H + 2 * oh) * (size_t)W + 2 * ow) * lanes + l;
        auto at = [&](int kd, int kh, int kw) { return base + (((size_t)kd * H + kh) * W + kw) * lanes; };
        float4 m = P::unpack(x[base]);
        int ix = 0, iy = 0, iz = 0, iw = 0;
#pragma unroll
        for (int k = 1; k < 8; k++) {
            const float4 v = P::unpack(x[at(k >> 2, (k >> 1) & 1, k & 1)]);
            if (v.x > m.x || v.x != v.x) { m.x = v.x; ix = k; }
            if (v.y > m.y || v.y != v.y) { m.y = v.y; iy = k; }
            if (v.z > m.z || v.z != v.z) { m.z = v.z; iz = k; }
            if (v.w > m.w || v.w != v.w) { m.w = v.w; iw = k; }
        }
        const float4 g = P::unpack(dy[o]);
        const int nd = 2 + ((od == OD - 1) & (D & 1)), nh = 2 + ((oh == OH - 1) & (H & 1));
        const int nw = 2 + ((ow == OW - 1) & (W & 1));
        for (int kd = 0; kd < nd; kd++)
            for (int kh = 0; kh < nh; kh++)
                for (int kw = 0; kw < nw; kw++) {
                    const int k = (kd < 2 && kh < 2 && kw < 2) ? kd * 4 + kh * 2 + kw : -1;   // -1: trailing voxel
                    dx[at(kd, kh, kw)] = P::pack(make_float4(ix == k ? g.x : 0.0f, iy == k ? g.y : 0.0f,
                                                             iz == k ? g.z : 0.0f, iw == k ? g.w : 0.0f));
                }
    }
}
template <typename T>
hipError_t launch_maxpool2_bwd_ndhwc(const T* x, const T* dy, T* dx, int batch, int D, int H, int W, int C,
                                     hipStream_t s) {
    using V = typename Pack<T>::type;
    const int OD = D / 2, OH = H / 2, OW = W / 2, lanes = C / 4;     // D, H, W >= 2 (checked by the caller)
    const size_t total = (size_t)batch * OD * OH * OW * lanes;
    if (total == 0) return hipSuccess;
    size_t blocks = (total + NG_THREADS - 1) / NG_THREADS;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(maxpool2_bwd_ndhwc_kernel<T>, dim3((unsigned)blocks), dim3(NG_THREADS), 0, s,
                       reinterpret_cast<const V*>(x), reinterpret_cast<const V*>(dy), reinterpret_cast<V*>(dx), total,
                       OD, OH, OW, D, H, W, lanes);
    return hipGetLastError();
}

// ---- trilinear x2 up-sampling backward (align_corners) -----------------------------------------------------
// The transpose of upsample2_ndhwc_kernel in gather form: one thread per INPUT voxel and four channels collects
// dy from the outputs that read the voxel.  Per axis those are the o with i0(o) == i or i1(o) == i; src = r o
// is monotone in o, so they form one run, at most 5 long (r < 1/2) and inside [2 i - 2, 2 i + 4]; the run is
// found by evaluating the forward's own up_axis on that window, so an output belongs to the run exactly when
// the forward read the voxel for it, with the forward's weight.  The sums are nested as the forward's lerps are
// (w, then h, then d), each in ascending o.  Extent 1 (out 2): both outputs have i0 = i1 = 0, weight 1.
// Half types: dy widened exactly, the sums in fp32 as for fp32 storage, dx rounded once.
__device__ __forceinline__ float up_weight(int o, int i, int in, float r) {
    const UpAxis a = up_axis(o, in, r);
    return (a.i0 == i ? a.w0 : 0.0f) + (a.i1 == i ? a.w1 : 0.0f);
}
__device__ __forceinline__ void up_run(int i, int in, float r, int& lo, int& hi) {
    lo = 1;
    hi = 0;
    const int a = 2 * i - 2 > 0 ? 2 * i - 2 : 0, z = 2 * i + 4 < 2 * in - 1 ? 2 * i + 4 : 2 * in - 1;
    bool found = false;
    for (int o = a; o <= z; o++) {
        const UpAxis ax = up_axis(o, in, r);
        if (ax.i0 == i || ax.i1 == i) {
            if (!found) lo = o;
            found = true;
            hi = o;
        }
    }
}
template <typename T>
__global__ __launch_bounds__(NG_THREADS) void upsample2_bwd_ndhwc_kernel(const typename Pack<T>::type* __restrict__ dy,
                                                                        typename Pack<T>::type* __restrict__ dx,
                                                                        size_t total, int D, int H, int W, int lanes,
                                                                        float rd, float rh, float rw) {
    using P = Pack<T>;
    const int OH = 2 * H, OW = 2 * W;
    for (size_t n = (size_t)blockIdx.x * NG_THREADS + threadIdx.x; n < total; n += (size_t)gridDim.x * NG_THREADS) {
        const int l = (int)(n % lanes);
        size_t t = n / lanes;
        const int w = (int)(t % W); t /= W;
        const int h = (int)(t % H); t /= H;
        const int d = (int)(t % D);
        const size_t b = t / D;
        int dlo, dhi, hlo, hhi, wlo, whi;
        up_run(d, D, rd, dlo, dhi);
        up_run(h, H, rh, hlo, hhi);
        up_run(w, W, rw, wlo, whi);
        const typename P::type* base = dy + (b * (2 * (size_t)D) * OH * OW) * lanes + l;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int od = dlo; od <= dhi; od++) {
            const float wd = up_weight(od, d, D, rd);
            float4 ah = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int oh = hlo; oh <= hhi; oh++) {
                const float wh = up_weight(oh, h, H, rh);
                float4 aw = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                for (int ow = wlo; ow <= whi; ow++) {
                    const float ww = up_weight(ow, w, W, rw);
                    const float4 g = P::unpack(base[(((size_t)od * OH + oh) * OW + ow) * lanes]);
                    aw.x = fmaf(ww, g.x, aw.x); aw.y = fmaf(ww, g.y, aw.y);
                    aw.z = fmaf(ww, g.z, aw.z); aw.w = fmaf(ww, g.w, aw.w);
                }
                ah.x = fmaf(wh, aw.x, ah.x); ah.y = fmaf(wh, aw.y, ah.y);
                ah.z = fmaf(wh, aw.z, ah.z); ah.w = fmaf(wh, aw.w, ah.w);
            }
            acc.x = fmaf(wd, ah.x, acc.x); acc.y = fmaf(wd, ah.y, acc.y);
            acc.z = fmaf(wd, ah.z, acc.z); acc.w = fmaf(wd, ah.w, acc.w);
        }
        dx[n] = P::pack(acc);
    }
}
template <typename T>
hipError_t launch_upsample2_trilinear_bwd_ndhwc(const T* dy, T* dx, int batch, int D, int H, int W, int C,
                                                hipStream_t s) {
    using V = typename Pack<T>::type;
    const int lanes = C / 4;
    const size_t total = (size_t)batch * D * H * (size_t)W * lanes;
    if (total == 0) return hipSuccess;
    size_t blocks = (total + NG_THREADS - 1) / NG_THREADS;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(upsample2_bwd_ndhwc_kernel<T>, dim3((unsigned)blocks), dim3(NG_THREADS), 0, s,
                       reinterpret_cast<const V*>(dy), reinterpret_cast<V*>(dx), total, D, H, W, lanes, up_ratio(D),
                       up_ratio(H), up_ratio(W));
    return hipGetLastError();
}

#define EXABM4D_NN_GRAD_INSTANTIATE(T)                                                                           \
    template hipError_t launch_groupnorm_lrelu_bwd_ndhwc<T>(const T*, const T*, const T*, T*, int, size_t, int,   \
                                                            int, const float*, const float*, float, float*,       \
                                                            float*, void*, hipStream_t);                          \
    template hipError_t launch_maxpool2_bwd_ndhwc<T>(const T*, const T*, T*, int, int, int, int, int, hipStream_t); \
    template hipError_t launch_upsample2_trilinear_bwd_ndhwc<T>(const T*, T*, int, int, int, int, int, hipStream_t);
EXABM4D_NN_GRAD_INSTANTIATE(float)
EXABM4D_NN_GRAD_INSTANTIATE(_Float16)
EXABM4D_NN_GRAD_INSTANTIATE(__bf16)
#undef EXABM4D_NN_GRAD_INSTANTIATE

// ---- foreground-weighted Charbonnier loss (reference machine_learning/losses.py) ---------------------------
// L = mean((1 + w m) sqrt(d^2 + eps^2)), d = pred - target, over n elements in storage order.  The loss is one
// number and its gradient one rounding per element, so each element is evaluated in fp64 (d is exact there) and
// rounded once; the pass stays bound by its 12 to 16 bytes per element.  M: the mask's storage, float or one
// byte (uint8 / bool); mask NULL: weight 1.
constexpr int CH_MAX_BLOCKS = 2048;
size_t charbonnier_workspace_bytes() { return CH_MAX_BLOCKS * sizeof(double); }

template <typename M>
__global__ __launch_bounds__(NG_THREADS) void charbonnier_partial_kernel(const float* __restrict__ pred,
                                                                        const float* __restrict__ target,
                                                                        const M* __restrict__ mask, size_t n,
                                                                        double w, double eps2,
                                                                        double* __restrict__ part) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * NG_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * NG_THREADS) {
        const double d = (double)pred[i] - (double)target[i];
        const double c = sqrt(fma(d, d, eps2));
        const double wt = mask ? fma(w, (double)mask[i], 1.0) : 1.0;
        acc = fma(wt, c, acc);
    }
    __shared__ double sh[NG_THREADS];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int k = NG_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(NG_THREADS) void charbonnier_final_kernel(const double* __restrict__ part, int nblk,
                                                                      double count, float* __restrict__ loss) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NG_THREADS) acc += part[i];
    __shared__ double sh[NG_THREADS];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int k = NG_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(sh[0] / count);
}
// dpred = g (1 + w m) d / sqrt(d^2 + eps^2) / n; g from device memory (under a GradScaler it is not 1).  A power
// of two in g scales every step exactly.
template <typename M>
__global__ __launch_bounds__(NG_THREADS) void charbonnier_bwd_kernel(const float* __restrict__ pred,
                                                                    const float* __restrict__ target,
                                                                    const M* __restrict__ mask, size_t n, double w,
                                                                    double eps2, double count,
                                                                    const float* __restrict__ grad_loss,
                                                                    float* __restrict__ dpred) {
    const double g = (double)grad_loss[0];
    for (size_t i = (size_t)blockIdx.x * NG_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * NG_THREADS) {
        const double d = (double)pred[i] - (double)target[i];
        const double c = sqrt(fma(d, d, eps2));
        const double wt = mask ? fma(w, (double)mask[i], 1.0) : 1.0;
        dpred[i] = (float)((g * wt) * d / c / count);
    }
}

static unsigned charbonnier_blocks(size_t n, size_t cap) {
    size_t blocks = (n + NG_THREADS - 1) / NG_THREADS;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}
hipError_t launch_charbonnier_loss(const float* pred, const float* target, const void* mask, int mask_bytes,
                                   size_t n, double w, double eps, void* workspace, float* loss, hipStream_t s) {
    double* part = static_cast<double*>(workspace);
    const unsigned blocks = charbonnier_blocks(n, CH_MAX_BLOCKS);
    if (mask_bytes == 4)
        hipLaunchKernelGGL(charbonnier_partial_kernel<float>, dim3(blocks), dim3(NG_THREADS), 0, s, pred, target,
                           static_cast<const float*>(mask), n, w, eps * eps, part);
    else
        hipLaunchKernelGGL(charbonnier_partial_kernel<uint8_t>, dim3(blocks), dim3(NG_THREADS), 0, s, pred, target,
                           static_cast<const uint8_t*>(mask), n, w, eps * eps, part);
    hipLaunchKernelGGL(charbonnier_final_kernel, dim3(1), dim3(NG_THREADS), 0, s, part, (int)blocks, (double)n, loss);
    return hipGetLastError();
}
hipError_t launch_charbonnier_loss_bwd(const float* pred, const float* target, const void* mask, int mask_bytes,
                                       size_t n, double w, double eps, const float* grad_loss, float* dpred,
                                       hipStream_t s) {
    const unsigned blocks = charbonnier_blocks(n, 65536);
    if (mask_bytes == 4)
        hipLaunchKernelGGL(charbonnier_bwd_kernel<float>, dim3(blocks), dim3(NG_THREADS), 0, s, pred, target,
                           static_cast<const float*>(mask), n, w, eps * eps, (double)n, grad_loss, dpred);
    else
        hipLaunchKernelGGL(charbonnier_bwd_kernel<uint8_t>, dim3(blocks), dim3(NG_THREADS), 0, s, pred, target,
                           static_cast<const uint8_t*>(mask), n, w, eps * eps, (double)n, grad_loss, dpred);
    return hipGetLastError();
}

}  // namespace exabm4d
