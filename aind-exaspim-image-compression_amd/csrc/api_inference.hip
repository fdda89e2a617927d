// api_inference.hip -- the BM4DNet stage's NDHWC GroupNorm, pooling and up-sampling, the intensity transforms and
// overlap tiling (what inference.py and transforms.py call).  Host code only; shared helpers: exabm4d_api.h.
#include <initializer_list>
#include <type_traits>

#include "exabm4d_api.h"

using namespace exabm4d;

// The prologue of the entries that take an exabm4d_transform: arguments, the transform's constants, the device.
static int tf_entry(exabm4d_ctx* ctx, bool ptrs_ok, const exabm4d_transform* t, TfDev& d) {
    if (!ctx || !ptrs_ok) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!t) return fail(ctx, EXABM4D_ERR_INVALID, "transform is NULL");
    if (t->size != sizeof(exabm4d_transform))
        return fail(ctx, EXABM4D_ERR_INVALID, "transform.size does not match this library");
    if (t->kind < 0 || t->kind > 2) return fail(ctx, EXABM4D_ERR_INVALID, "unknown transform kind");
    std::memset(&d, 0, sizeof d);
    d.kind = t->kind;
    d.wrapped = t->wrapped ? 1 : 0;
    d.woff = (float)t->wrap_offset;
    d.maxc = (float)t->max_count;
    d.off = (float)t->offset;
    d.scale = (float)t->scale;
    d.norm = (float)t->norm;
    d.gain = (float)t->gain;
    d.c38g2 = (float)((3.0 / 8.0) * t->gain * t->gain);
    d.rn2 = (float)(t->read_noise * t->read_noise);
    d.two_over_gain = (float)(2.0 / t->gain);
    d.cinvg2 = (float)(t->c_inv * t->gain * t->gain);
    d.mn = (float)t->mn;
    d.fden = (float)(t->mx - t->mn + 1e-8);
    d.clip = (float)t->clip;
    d.range = (float)(t->mx - t->mn);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return EXABM4D_OK;
}

// The fp32 entries are the dtype-coded ones with EXABM4D_DTYPE_F32; the element type picks the template
// instance of nn_kernels.hip (_Float16 / __bf16 storage for fp16 / bf16, 8-byte four-channel vectors).
static bool nn_dtype_ok(int dtype) {
    return dtype == EXABM4D_DTYPE_F32 || dtype == EXABM4D_DTYPE_F16 || dtype == EXABM4D_DTYPE_BF16;
}
static uintptr_t nn_align_mask(int dtype) { return dtype == EXABM4D_DTYPE_F32 ? 15u : 7u; }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// whether every tensor of `ps` has the alignment its element type needs, and the message for when one has not
static bool nn_aligned(int dtype, std::initializer_list<const void*> ps) {
    uintptr_t bits = 0;
    for (const void* p : ps) bits |= (uintptr_t)p;
    return (bits & nn_align_mask(dtype)) == 0;
}
static const char* nn_align_msg(int dtype, const char* f32, const char* half) {
    return dtype == EXABM4D_DTYPE_F32 ? f32 : half;
}
// Calls f with a null pointer of the element type of `dtype` (nn_dtype_ok), which picks the launcher's instance.
template <typename F>
static hipError_t nn_dispatch(int dtype, F&& f) {
    if (dtype == EXABM4D_DTYPE_F32) return f(static_cast<float*>(nullptr));
    if (dtype == EXABM4D_DTYPE_F16) return f(static_cast<_Float16*>(nullptr));
    return f(static_cast<__bf16*>(nullptr));
}

extern "C" {

// ---- BM4DNet stage: fused GroupNorm + LeakyReLU on NDHWC tensors (nn_kernels.hip) ------------------------
size_t exabm4d_groupnorm_workspace_bytes(int batch, size_t spatial, int channels, int groups) {
    if (batch < 1 || channels < 1 || groups < 1) return 0;
    return groupnorm_workspace_bytes(batch, spatial, channels, groups);
}
int exabm4d_groupnorm_lrelu_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                         int batch, size_t spatial, int channels, int groups, const float* gamma,
                                         const float* beta, float eps, float slope, void* workspace,
                                         size_t workspace_bytes, const float* conv_bias) {
    if (!ctx || !x || !y || !workspace) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!nn_dtype_ok(dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_ndhwc: unknown dtype");
    if (conv_bias && !aligned16(conv_bias))
        return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_ndhwc: conv_bias must be 16-byte aligned");
    if (batch < 1 || batch > 65535 || spatial < 1 || channels < 4 || groups < 1 || groups > 32 ||
        channels % groups != 0 || channels % 4 != 0 || (channels / groups) % 4 != 0 || 256 % (channels / 4) != 0)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED,
                    "groupnorm_lrelu_ndhwc: needs channels % 4 == 0, (channels / groups) % 4 == 0, "
                    "256 % (channels / 4) == 0 and groups <= 32 (use the framework's GroupNorm otherwise)");
    if (workspace_bytes < groupnorm_workspace_bytes(batch, spatial, channels, groups))
        return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_ndhwc: workspace too small");
    if (!nn_aligned(dtype, {x, y}) || !aligned16(workspace))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    nn_align_msg(dtype, "groupnorm_lrelu_ndhwc: 16-byte aligned tensors expected",
                                 "groupnorm_lrelu_ndhwc: 8-byte aligned tensors and a 16-byte aligned workspace "
                                 "expected"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_groupnorm_lrelu_ndhwc(static_cast<const T*>(x), static_cast<T*>(y), batch, spatial, channels,
                                            groups, gamma, beta, eps, slope, workspace, (hipStream_t)hip_stream,
                                            conv_bias);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_groupnorm_lrelu_ndhwc");
}
int exabm4d_groupnorm_lrelu_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                      size_t spatial, int channels, int groups, const float* gamma,
                                      const float* beta, float eps, float slope, void* workspace,
                                      size_t workspace_bytes, const float* conv_bias) {
    return exabm4d_groupnorm_lrelu_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, y, batch, spatial, channels,
                                                groups, gamma, beta, eps, slope, workspace, workspace_bytes,
                                                conv_bias);
}

static int nn_resample_checks(exabm4d_ctx* ctx, int dtype, const void* x, const void* y, int batch, int d, int h,
                              int w, int channels) {
    if (!ctx || !x || !y) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!nn_dtype_ok(dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "NDHWC resampling: unknown dtype");
    if (batch < 1 || d < 1 || h < 1 || w < 1 || channels < 4 || channels % 4 != 0)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "NDHWC resampling: sizes >= 1 and channels % 4 == 0");
    if (!nn_aligned(dtype, {x, y}))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    nn_align_msg(dtype, "NDHWC resampling: 16-byte aligned tensors expected",
                                 "NDHWC resampling: 8-byte aligned tensors expected"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return EXABM4D_OK;
}
int exabm4d_maxpool2_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y, int batch,
                                  int d, int h, int w, int channels) {
    int rc = nn_resample_checks(ctx, dtype, x, y, batch, d, h, w, channels);
    if (rc) return rc;
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_maxpool2_ndhwc(static_cast<const T*>(x), static_cast<T*>(y), batch, d, h, w, channels,
                                     (hipStream_t)hip_stream);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_maxpool2_ndhwc");
}
int exabm4d_upsample2_trilinear_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                             int batch, int d, int h, int w, int channels) {
    int rc = nn_resample_checks(ctx, dtype, x, y, batch, d, h, w, channels);
    if (rc) return rc;
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_upsample2_trilinear_ndhwc(static_cast<const T*>(x), static_cast<T*>(y), batch, d, h, w,
                                                channels, (hipStream_t)hip_stream);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_upsample2_trilinear_ndhwc");
}
int exabm4d_maxpool2_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch, int d,
                               int h, int w, int channels) {
    return exabm4d_maxpool2_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, y, batch, d, h, w, channels);
}
int exabm4d_upsample2_trilinear_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                          int d, int h, int w, int channels) {
    return exabm4d_upsample2_trilinear_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, y, batch, d, h, w,
                                                    channels);
}

// ---- BM4DNet training: the forward that keeps its statistics, the three backward passes (each dtype-coded like
// the forward entries, the fp32 ones being these with EXABM4D_DTYPE_F32), the loss (nn_grad_kernels.hip)
static int gn_shape_checks(exabm4d_ctx* ctx, int batch, size_t spatial, int channels, int groups, const char* unsup) {
    if (batch < 1 || batch > 65535 || spatial < 1 || channels < 4 || groups < 1 || groups > 32 ||
        channels % groups != 0 || channels % 4 != 0 || (channels / groups) % 4 != 0 || 256 % (channels / 4) != 0)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, unsup);
    return EXABM4D_OK;
}
int exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                               int batch, size_t spatial, int channels, int groups,
                                               const float* gamma, const float* beta, float eps, float slope,
                                               void* workspace, size_t workspace_bytes, float* mean_rstd) {
    if (!ctx || !x || !y || !workspace || !mean_rstd) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!nn_dtype_ok(dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_ndhwc_train: unknown dtype");
    if (int rc = gn_shape_checks(ctx, batch, spatial, channels, groups,
                                 "groupnorm_lrelu_ndhwc_train: needs channels % 4 == 0, (channels / groups) % 4 == 0, "
                                 "256 % (channels / 4) == 0 and groups <= 32"))
        return rc;
    if (!(slope > 0.0f))
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED,
                    "groupnorm_lrelu_ndhwc_train: slope must be > 0 (the backward reads the side from y)");
    if (workspace_bytes < groupnorm_workspace_bytes(batch, spatial, channels, groups))
        return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_ndhwc_train: workspace too small");
    if (!nn_aligned(dtype, {x, y}) || !aligned16(workspace))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    nn_align_msg(dtype, "groupnorm_lrelu_ndhwc_train: 16-byte aligned tensors expected",
                                 "groupnorm_lrelu_ndhwc_train: 8-byte aligned tensors and a 16-byte aligned "
                                 "workspace expected"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_groupnorm_lrelu_ndhwc(static_cast<const T*>(x), static_cast<T*>(y), batch, spatial, channels,
                                            groups, gamma, beta, eps, slope, workspace, (hipStream_t)hip_stream,
                                            nullptr, mean_rstd);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_groupnorm_lrelu_ndhwc");
}
int exabm4d_groupnorm_lrelu_ndhwc_train_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                            size_t spatial, int channels, int groups, const float* gamma,
                                            const float* beta, float eps, float slope, void* workspace,
                                            size_t workspace_bytes, float* mean_rstd) {
    return exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, y, batch, spatial,
                                                      channels, groups, gamma, beta, eps, slope, workspace,
                                                      workspace_bytes, mean_rstd);
}
size_t exabm4d_groupnorm_lrelu_bwd_workspace_bytes(int batch, size_t spatial, int channels, int groups) {
    if (batch < 1 || spatial < 1 || channels < 4 || groups < 1 || channels % 4 != 0 || 256 % (channels / 4) != 0)
        return 0;
    return groupnorm_bwd_workspace_bytes(batch, spatial, channels, groups);
}
int exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x,
                                             const void* y, const void* dy, void* dx, int batch, size_t spatial,
                                             int channels, int groups, const float* gamma, const float* mean_rstd,
                                             float slope, float* dgamma, float* dbeta, void* workspace,
                                             size_t workspace_bytes) {
    if (!ctx || !x || !y || !dy || !dx || !mean_rstd || !workspace)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!nn_dtype_ok(dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_bwd_ndhwc: unknown dtype");
    if (int rc = gn_shape_checks(ctx, batch, spatial, channels, groups,
                                 "groupnorm_lrelu_bwd_ndhwc: needs channels % 4 == 0, (channels / groups) % 4 == 0, "
                                 "256 % (channels / 4) == 0 and groups <= 32"))
        return rc;
    if (!(slope > 0.0f))
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED,
                    "groupnorm_lrelu_bwd_ndhwc: slope must be > 0 (the activation's side is read from y)");
    if (workspace_bytes < groupnorm_bwd_workspace_bytes(batch, spatial, channels, groups))
        return fail(ctx, EXABM4D_ERR_INVALID, "groupnorm_lrelu_bwd_ndhwc: workspace too small");
    if (!nn_aligned(dtype, {x, y, dy, dx}) || !aligned16(workspace))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    nn_align_msg(dtype, "groupnorm_lrelu_bwd_ndhwc: 16-byte aligned tensors expected",
                                 "groupnorm_lrelu_bwd_ndhwc: 8-byte aligned tensors and a 16-byte aligned "
                                 "workspace expected"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_groupnorm_lrelu_bwd_ndhwc(static_cast<const T*>(x), static_cast<const T*>(y),
                                                static_cast<const T*>(dy), static_cast<T*>(dx), batch, spatial,
                                                channels, groups, gamma, mean_rstd, slope, dgamma, dbeta, workspace,
                                                (hipStream_t)hip_stream);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_groupnorm_lrelu_bwd_ndhwc");
}
int exabm4d_groupnorm_lrelu_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, const float* y,
                                          const float* dy, float* dx, int batch, size_t spatial, int channels,
                                          int groups, const float* gamma, const float* mean_rstd, float slope,
                                          float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes) {
    return exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, y, dy, dx, batch, spatial,
                                                    channels, groups, gamma, mean_rstd, slope, dgamma, dbeta,
                                                    workspace, workspace_bytes);
}
int exabm4d_maxpool2_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, const void* dy,
                                      void* dx, int batch, int d, int h, int w, int channels) {
    if (!dy) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (int rc = nn_resample_checks(ctx, dtype, x, dx, batch, d, h, w, channels)) return rc;
    if (d < 2 || h < 2 || w < 2) return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "maxpool2_bwd_ndhwc: extents >= 2");
    if (!nn_aligned(dtype, {dy}))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    nn_align_msg(dtype, "NDHWC resampling: 16-byte aligned tensors expected",
                                 "NDHWC resampling: 8-byte aligned tensors expected"));
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_maxpool2_bwd_ndhwc(static_cast<const T*>(x), static_cast<const T*>(dy), static_cast<T*>(dx),
                                         batch, d, h, w, channels, (hipStream_t)hip_stream);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_maxpool2_bwd_ndhwc");
}
int exabm4d_maxpool2_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, const float* dy, float* dx,
                                   int batch, int d, int h, int w, int channels) {
    return exabm4d_maxpool2_bwd_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, x, dy, dx, batch, d, h, w, channels);
}
int exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* dy,
                                                 void* dx, int batch, int d, int h, int w, int channels) {
    if (int rc = nn_resample_checks(ctx, dtype, dy, dx, batch, d, h, w, channels)) return rc;
    const hipError_t e = nn_dispatch(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch_upsample2_trilinear_bwd_ndhwc(static_cast<const T*>(dy), static_cast<T*>(dx), batch, d, h, w,
                                                    channels, (hipStream_t)hip_stream);
    });
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_upsample2_trilinear_bwd_ndhwc");
}
int exabm4d_upsample2_trilinear_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* dy, float* dx,
                                              int batch, int d, int h, int w, int channels) {
    return exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(ctx, hip_stream, EXABM4D_DTYPE_F32, dy, dx, batch, d, h, w,
                                                        channels);
}
size_t exabm4d_charbonnier_workspace_bytes(void) { return charbonnier_workspace_bytes(); }
static int charbonnier_checks(exabm4d_ctx* ctx, bool ptrs_ok, int mask_bytes, size_t n, double fg_weight, double eps) {
    if (!ctx || !ptrs_ok) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (mask_bytes != 1 && mask_bytes != 4)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "charbonnier_loss: mask elements of 1 (uint8 / bool) or 4 (fp32) bytes");
    if (n < 1 || !(eps >= 0.0) || fg_weight != fg_weight)
        return fail(ctx, EXABM4D_ERR_INVALID, "charbonnier_loss: n >= 1, eps >= 0 and a fg_weight that is a number");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return EXABM4D_OK;
}
int exabm4d_charbonnier_loss_dev(exabm4d_ctx* ctx, void* hip_stream, const float* pred, const float* target,
                                 const void* mask, int mask_bytes, size_t n, double fg_weight, double eps,
                                 void* workspace, size_t workspace_bytes, float* loss) {
    if (int rc = charbonnier_checks(ctx, pred && target && workspace && loss, mask_bytes, n, fg_weight, eps)) return rc;
    if (workspace_bytes < charbonnier_workspace_bytes() || ((uintptr_t)workspace & 7u) != 0)
        return fail(ctx, EXABM4D_ERR_INVALID, "charbonnier_loss: workspace too small or not 8-byte aligned");
    const hipError_t e = launch_charbonnier_loss(pred, target, mask, mask_bytes, n, fg_weight, eps, workspace, loss,
                                                 (hipStream_t)hip_stream);
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_charbonnier_loss");
}
int exabm4d_charbonnier_loss_bwd_dev(exabm4d_ctx* ctx, void* hip_stream, const float* pred, const float* target,
                                     const void* mask, int mask_bytes, size_t n, double fg_weight, double eps,
                                     const float* grad_loss, float* dpred) {
    if (int rc = charbonnier_checks(ctx, pred && target && grad_loss && dpred, mask_bytes, n, fg_weight, eps)) return rc;
    const hipError_t e = launch_charbonnier_loss_bwd(pred, target, mask, mask_bytes, n, fg_weight, eps, grad_loss,
                                                     dpred, (hipStream_t)hip_stream);
    return e == hipSuccess ? EXABM4D_OK : fail_hip(ctx, e, "launch_charbonnier_loss_bwd");
}

// ---- intensity transforms ---------------------------------------------------------------------------------
int exabm4d_transform_forward_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const uint16_t* in, float* out, size_t n) {
    TfDev d;
    if (int rc = tf_entry(ctx, in && out, t, d)) return rc;
    if (d.kind == EXABM4D_TF_ASINH && n >= ((size_t)1 << 20)) {
        // asinh is evaluated in fp64: large uint16 volumes go through a 65536-entry table
        if (!ctx->tf_lut.p) {
            HIP_TRY(ctx, hipMalloc(&ctx->tf_lut.p, 65536 * sizeof(float)));
            ctx->tf_lut.bytes = 65536 * sizeof(float);
        }
        HIP_TRY(ctx, launch_tf_forward_u16_lut(d, ctx->tf_lut.as<float>(), in, out, n, ctx->stream));
        return EXABM4D_OK;
    }
    HIP_TRY(ctx, launch_tf_forward_u16(d, in, out, n, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_transform_forward_f32_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, float* out, size_t n) {
    TfDev d;
    if (int rc = tf_entry(ctx, in && out, t, d)) return rc;
    HIP_TRY(ctx, launch_tf_forward_f32(d, in, out, n, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_transform_inverse_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, uint16_t* out, size_t n) {
    TfDev d;
    if (int rc = tf_entry(ctx, in && out, t, d)) return rc;
    HIP_TRY(ctx, launch_tf_inverse(d, in, out, n, 1, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_transform_inverse_f32_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, float* out, size_t n) {
    TfDev d;
    if (int rc = tf_entry(ctx, in && out, t, d)) return rc;
    HIP_TRY(ctx, launch_tf_inverse(d, in, out, n, 0, ctx->stream));
    return EXABM4D_OK;
}

// ---- overlap tiling ---------------------------------------------------------------------------------------------
int exabm4d_tile_gather_dev(exabm4d_ctx* ctx, const float* vol, int nz, int ny, int nx,
                            const int32_t* starts, int nb, int patch, float* out) {
    if (!ctx || !vol || !starts || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nb < 0 || patch < 1 || nz < 1 || ny < 1 || nx < 1) return fail(ctx, EXABM4D_ERR_INVALID, "bad sizes");
    for (int i = 0; i < 3 * nb; i++)
        if (starts[i] < 0) return fail(ctx, EXABM4D_ERR_INVALID, "negative patch start");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_tile_gather(vol, nz, ny, nx, starts, nb, patch, out, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_tile_accumulate_dev(exabm4d_ctx* ctx, const float* preds, const int32_t* starts, int nb,
                                int patch, int trim, float* accum_pred, float* accum_wgt, int nz,
                                int ny, int nx) {
    if (!ctx || !preds || !starts || !accum_pred || !accum_wgt)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nb < 0 || patch < 1 || trim < 0 || 2 * trim >= patch) return fail(ctx, EXABM4D_ERR_INVALID, "bad sizes");
    for (int i = 0; i < 3 * nb; i++)
        if (starts[i] < 0) return fail(ctx, EXABM4D_ERR_INVALID, "negative patch start");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_tile_accumulate(preds, starts, nb, patch, trim, accum_pred, accum_wgt, nz, ny,
                                        nx, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_tile_finalize_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                  const float* accum_pred, const float* accum_wgt, uint16_t* out,
                                  size_t n) {
    TfDev d;
    if (int rc = tf_entry(ctx, accum_pred && accum_wgt && out, t, d)) return rc;
    HIP_TRY(ctx, launch_tile_finalize(d, accum_pred, accum_wgt, out, n, ctx->stream));
    return EXABM4D_OK;
}

// ---- overlap tiling of one brick -----------------------------------------------------------------
// The grid as the kernels take it, or false: sizes in range and every patch's far end inside int.
static bool tile_grid(const exabm4d_patch_grid* grid, TileGrid& g, long long& patches) {
    if (!grid || grid->stride < 1 || grid->patch < 1 || grid->patch > 1024) return false;
    patches = 1;
    for (int a = 0; a < 3; a++) {
        if (grid->first[a] < 0 || grid->count[a] < 0) return false;
        const long long end = ((long long)grid->first[a] + grid->count[a]) * grid->stride + grid->patch;
        if (end > 0x7fffffffLL) return false;
        g.first[a] = grid->first[a];
        g.count[a] = grid->count[a];
        patches *= grid->count[a];
        if (patches > (1LL << 40)) return false;                 // checked per factor: the product cannot wrap
    }
    g.stride = grid->stride;
    g.patch = grid->patch;
    return true;
}
int exabm4d_tile_gather_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* win_origin_zyx,
                                const int32_t* win_dims_zyx, const int32_t* vol_dims_zyx,
                                const exabm4d_transform* t, const exabm4d_patch_grid* grid, long long k0, int nb,
                                float* out) {
    TfDev d;
    if (int rc = tf_entry(ctx, win && win_origin_zyx && win_dims_zyx && vol_dims_zyx && grid && out, t, d)) return rc;
    TileGrid g;
    long long patches = 0;
    if (!tile_grid(grid, g, patches)) return fail(ctx, EXABM4D_ERR_INVALID, "tile_gather_u16: bad patch grid");
    if (k0 < 0 || nb < 0 || k0 + nb > patches)
        return fail(ctx, EXABM4D_ERR_INVALID, "tile_gather_u16: the batch runs past the patch grid");
    Int3 w0, wd, vol;
    for (int a = 0; a < 3; a++) {
        w0.v[a] = win_origin_zyx[a];
        wd.v[a] = win_dims_zyx[a];
        vol.v[a] = vol_dims_zyx[a];
        if (w0.v[a] < 0 || wd.v[a] < 1 || vol.v[a] < 1) return fail(ctx, EXABM4D_ERR_INVALID, "tile_gather_u16: bad sizes");
        if (g.count[a] == 0) continue;
        const long long lo = (long long)g.first[a] * g.stride;
        const long long hi = std::min<long long>(((long long)g.first[a] + g.count[a] - 1) * g.stride + g.patch, vol.v[a]);
        if (lo < hi && (w0.v[a] > lo || hi > (long long)w0.v[a] + wd.v[a]))
            return fail(ctx, EXABM4D_ERR_INVALID, "tile_gather_u16: the window does not hold the grid's patches");
    }
    HIP_TRY(ctx, launch_tile_gather_u16(win, w0, wd, vol, d, g, k0, nb, out, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_tile_stitch_u16_dev(exabm4d_ctx* ctx, const float* preds, long long n_patches,
                                const exabm4d_patch_grid* grid, int trim, const int32_t* box_origin_zyx,
                                const int32_t* box_dims_zyx, const int32_t* vol_dims_zyx,
                                const exabm4d_transform* t, uint16_t* out) {
    TfDev d;
    if (int rc = tf_entry(ctx, grid && box_origin_zyx && box_dims_zyx && vol_dims_zyx && out, t, d)) return rc;
    TileGrid g;
    long long patches = 0;
    if (!tile_grid(grid, g, patches)) return fail(ctx, EXABM4D_ERR_INVALID, "tile_stitch_u16: bad patch grid");
    if (n_patches != patches || (patches > 0 && !preds))
        return fail(ctx, EXABM4D_ERR_INVALID, "tile_stitch_u16: preds does not hold the grid's patches");
    if (trim < 0 || 2 * trim >= g.patch) return fail(ctx, EXABM4D_ERR_INVALID, "tile_stitch_u16: 0 <= 2 trim < patch");
    Int3 o0, oe;
    for (int a = 0; a < 3; a++) {
        o0.v[a] = box_origin_zyx[a];
        oe.v[a] = box_dims_zyx[a];
        if (o0.v[a] < 0 || oe.v[a] < 1 || (long long)o0.v[a] + oe.v[a] > vol_dims_zyx[a])
            return fail(ctx, EXABM4D_ERR_INVALID, "tile_stitch_u16: the box is not inside the volume");
    }
    HIP_TRY(ctx, launch_tile_stitch_u16(preds, g, trim, o0, oe, d, out, ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
