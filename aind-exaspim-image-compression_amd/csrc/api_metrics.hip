// api_metrics.hip -- histograms, min / max, error statistics, SSIM, the patch-cache foreground masks and the
// coherence gate.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

extern "C" {

// ---- background offset + quality metrics (row f-4) ---------------------------------------------------
static bool bad_dtype(int d) { return d < EXABM4D_DT_U16 || d > EXABM4D_DT_F64; }

int exabm4d_u16_histogram_dev(exabm4d_ctx* ctx, const uint16_t* vol, size_t n, uint64_t* hist_host) {
    if (!ctx || !hist_host || (!vol && n)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = grow(ctx, ctx->red, 65536 * sizeof(uint64_t))) return rc;
    HIP_TRY(ctx, launch_hist_u16(vol, n, ctx->red.as<unsigned long long>(), ctx->stream));
    return fetch(ctx, hist_host, ctx->red.p, 65536 * sizeof(uint64_t));
}

int exabm4d_i32_symbol_histogram_dev(exabm4d_ctx* ctx, const int32_t* idx, size_t n, uint64_t* hist_host) {
    if (!ctx || !hist_host || (!idx && n)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = grow(ctx, ctx->red, 65536 * sizeof(uint64_t))) return rc;
    HIP_TRY(ctx, launch_hist_i32_clamped(idx, n, ctx->red.as<unsigned long long>(), ctx->stream));
    return fetch(ctx, hist_host, ctx->red.p, 65536 * sizeof(uint64_t));
}

int exabm4d_key_histogram_dev(exabm4d_ctx* ctx, const void* vol, int dtype, size_t n, int absdev,
                              double center, int digit, uint64_t prefix, uint64_t* hist_host) {
    if (!ctx || !hist_host || (!vol && n)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_dtype(dtype) || digit < 0 || digit > 3) return fail(ctx, EXABM4D_ERR_INVALID, "bad dtype / digit");
    if (digit > 0 && digit < 4 && (prefix >> (16 * digit)) != 0)
        return fail(ctx, EXABM4D_ERR_INVALID, "prefix wider than the digits above");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = grow(ctx, ctx->red, 65536 * sizeof(uint64_t))) return rc;
    HIP_TRY(ctx, launch_hist_key(vol, dtype, n, absdev ? 1 : 0, center, digit,
                                 (unsigned long long)prefix, ctx->red.as<unsigned long long>(),
                                 ctx->stream));
    return fetch(ctx, hist_host, ctx->red.p, 65536 * sizeof(uint64_t));
}

int exabm4d_minmax_dev(exabm4d_ctx* ctx, const void* vol, int dtype, size_t n, double* out_host) {
    if (!ctx || !vol || !out_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_dtype(dtype) || n == 0) return fail(ctx, EXABM4D_ERR_INVALID, "bad dtype / empty input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)masked_stats_partials(n) * 2;
    if (int rc = grow(ctx, ctx->red, (np + 2) * sizeof(double))) return rc;
    double* d = ctx->red.as<double>();
    HIP_TRY(ctx, launch_minmax(vol, dtype, n, d + 2, d, ctx->stream));
    return fetch(ctx, out_host, d, 2 * sizeof(double));
}

int exabm4d_masked_error_stats_dev(exabm4d_ctx* ctx, const void* pred, int pred_dtype,
                                   const void* ref, int ref_dtype, const uint8_t* mask, size_t n,
                                   double thr, double* out_host) {
    if (!ctx || !pred || !ref || !out_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_dtype(pred_dtype) || bad_dtype(ref_dtype) || n == 0)
        return fail(ctx, EXABM4D_ERR_INVALID, "bad dtype / empty input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)masked_stats_partials(n) * 7;
    if (int rc = grow(ctx, ctx->red, (np + 8) * sizeof(double))) return rc;
    double* d = ctx->red.as<double>();
    HIP_TRY(ctx, launch_masked_stats(pred, pred_dtype, ref, ref_dtype, mask, n, thr, d + 8, d,
                                     ctx->stream));
    return fetch(ctx, out_host, d, 7 * sizeof(double));
}

int exabm4d_ssim3d_dev(exabm4d_ctx* ctx, const void* a, const void* b, int dtype, int nz, int ny,
                       int nx, int window, double c1, double c2, double* sum_host) {
    if (!ctx || !a || !b || !sum_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_dtype(dtype) || nz < 1 || ny < 1 || nx < 1) return fail(ctx, EXABM4D_ERR_INVALID, "bad dtype / sizes");
    if (window < 1 || window > ssim3d_max_window())
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "ssim window must be 1..32");
    if ((long long)nz * ny * nx > (1ll << 40) || nz > (1 << 20) || ny > (1 << 20) || nx > (1 << 20))
        return fail(ctx, EXABM4D_ERR_INVALID, "volume too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)ssim3d_partials(nz, ny, nx);
    if (int rc = grow(ctx, ctx->red, (np + 1) * sizeof(double))) return rc;
    double* d = ctx->red.as<double>();
    HIP_TRY(ctx, launch_ssim3d(a, b, dtype, nz, ny, nx, window, c1, c2, d + 1, d, ctx->stream));
    return fetch(ctx, sum_host, d, sizeof(double));
}

// ---- noise table ---------------------------------------------------------------------
static_assert(NOISE_LEVELS == EXABM4D_NOISE_LEVELS && NOISE_BINS == EXABM4D_NOISE_BINS,
              "exabm4d.h and exabm4d_kernels.h differ");

int exabm4d_noise_table_dev(exabm4d_ctx* ctx, const void* vol, int dtype, int nz, int ny, int nx, int shift,
                            uint64_t* hist_host, uint64_t* sum_s_host, uint64_t* skipped_host) {
    if (!ctx || !vol || !hist_host || !sum_s_host || !skipped_host)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (dtype != EXABM4D_DT_U16 && dtype != EXABM4D_DT_F32)
        return fail(ctx, EXABM4D_ERR_INVALID, "vol must be uint16 or float32");
    if (shift < 0 || shift > 6) return fail(ctx, EXABM4D_ERR_INVALID, "shift must be 0..6");
    if (nz < 2 || ny < 2 || nx < 2) return fail(ctx, EXABM4D_ERR_INVALID, "every extent must be >= 2");
    if ((long long)nz * ny * nx > (1ll << 40) || (long long)(nz / 2) * (ny / 2) >= (1ll << 31))
        return fail(ctx, EXABM4D_ERR_INVALID, "volume too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = grow(ctx, ctx->red, noise_table_bytes())) return rc;
    unsigned long long* d = ctx->red.as<unsigned long long>();
    if (!ctx->noise_wgs) HIP_TRY(ctx, noise_table_prepare(ctx->device, &ctx->noise_wgs));
    HIP_TRY(ctx, launch_noise_table(vol, dtype, nz, ny, nx, shift, ctx->noise_wgs, d, ctx->stream));
    const size_t nh = (size_t)NOISE_LEVELS * NOISE_BINS;
    HIP_TRY(ctx, hipMemcpyAsync(hist_host, d, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(sum_s_host, d + nh, NOISE_LEVELS * 8, hipMemcpyDeviceToHost, ctx->stream));
    return fetch(ctx, skipped_host, d + nh + NOISE_LEVELS, 8);
}

// ---- patch-cache foreground masks and coherence gate ---------------------------------
// check_patches and bad_label_dtype are shared with api_sampler.hip (exabm4d_api.h)
static_assert(LS_MAX == EXABM4D_LABEL_SET_MAX && SEG_STATS_K == EXABM4D_SEG_STATS_K &&
              GF_MAXR == EXABM4D_GAUSS_MAX_RADIUS && LBL_I64 == EXABM4D_LBL_I64, "exabm4d.h and exabm4d_kernels.h differ");

int exabm4d_foreground_masks_dev(exabm4d_ctx* ctx, const void* raw, int dtype, int batch, int nz, int ny,
                                 int nx, float k, int dilate, uint8_t* mask, float* thr_host) {
    if (!ctx || !raw || !mask) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (dtype != EXABM4D_DT_U16 && dtype != EXABM4D_DT_F32)
        return fail(ctx, EXABM4D_ERR_INVALID, "raw must be uint16 or float32");
    if (dilate < 0) return fail(ctx, EXABM4D_ERR_INVALID, "dilate must be >= 0");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)nz * ny * nx * batch;
    struct { float* thr; uint8_t* tmp; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.thr = c.take<float>((size_t)batch * sizeof(float));
            r.tmp = c.take<uint8_t>(dilate > 1 ? total : 0);
        }))
        return rc;
    HIP_TRY(ctx, launch_fg_threshold(raw, dtype, batch, (size_t)nz * ny * nx, k, L.thr, ctx->stream));
    HIP_TRY(ctx, launch_dilate(nullptr, raw, dtype, L.thr, batch, nz, ny, nx, dilate, L.tmp, mask, ctx->stream));
    if (thr_host) return fetch(ctx, thr_host, L.thr, (size_t)batch * sizeof(float));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_binary_dilate_dev(exabm4d_ctx* ctx, const uint8_t* in, int batch, int nz, int ny, int nx,
                              int iterations, uint8_t* out) {
    if (!ctx || !in || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (in == out) return fail(ctx, EXABM4D_ERR_INVALID, "in and out must be distinct");
    if (iterations < 0) return fail(ctx, EXABM4D_ERR_INVALID, "iterations must be >= 0");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)nz * ny * nx * batch;
    if (iterations > 1)
        if (int rc = grow(ctx, ctx->red, total)) return rc;
    HIP_TRY(ctx, launch_dilate(in, nullptr, 0, nullptr, batch, nz, ny, nx, iterations, ctx->red.as<uint8_t>(), out,
                               ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_gaussian_filter3d_dev(exabm4d_ctx* ctx, const void* src, int dtype, int batch, int nz, int ny,
                                  int nx, const double* weights_host, int radius, double* out) {
    if (!ctx || !src || !weights_host || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (dtype != EXABM4D_DT_F32 && dtype != EXABM4D_DT_F64)
        return fail(ctx, EXABM4D_ERR_INVALID, "src must be float32 or float64");
    if (src == out) return fail(ctx, EXABM4D_ERR_INVALID, "src and out must be distinct");
    if (radius < 0 || radius > EXABM4D_GAUSS_MAX_RADIUS)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "gaussian radius must be 0..EXABM4D_GAUSS_MAX_RADIUS");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GaussWeights w{};
    w.radius = radius;
    for (int j = 0; j <= radius; j++) w.w[j] = weights_host[j];
    const size_t total = (size_t)nz * ny * nx * batch;
    if (int rc = grow(ctx, ctx->red, total * sizeof(double))) return rc;
    HIP_TRY(ctx, launch_gaussian3d(src, dtype, batch, nz, ny, nx, w, ctx->red.as<double>(), out, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_label_set_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, int batch, int nz, int ny,
                          int nx, uint64_t* keys_host, uint32_t* counts_host, uint32_t* n_host,
                          uint32_t* status_host) {
    if (!ctx || !labels || !keys_host || !counts_host || !n_host || !status_host)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_label_dtype(label_dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "bad label dtype");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nk = (size_t)batch * LS_MAX;
    struct { unsigned long long* keys; uint32_t *counts, *n, *status; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.keys = c.take<unsigned long long>(nk * 8);
            r.counts = c.take<uint32_t>(nk * 4);
            r.n = c.take<uint32_t>((size_t)batch * 4);
            r.status = c.take<uint32_t>((size_t)batch * 4);
        }))
        return rc;
    HIP_TRY(ctx, launch_label_set(labels, label_dtype, batch, (size_t)nz * ny * nx, L.keys, L.counts, L.n, L.status,
                                  ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(keys_host, L.keys, nk * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(counts_host, L.counts, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_host, L.n, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
    return fetch(ctx, status_host, L.status, (size_t)batch * 4);
}

int exabm4d_segment_stats_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, const void* raw,
                              int raw_dtype, const double* smooth, int batch, int nz, int ny, int nx, int lag,
                              const int32_t* item_patch_host, const uint64_t* item_key_host, int n_items,
                              double* out_host) {
    if (!ctx || !labels || !raw || (n_items > 0 && (!item_patch_host || !item_key_host || !out_host)))
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (bad_label_dtype(label_dtype) || (raw_dtype != EXABM4D_DT_F32 && raw_dtype != EXABM4D_DT_F64))
        return fail(ctx, EXABM4D_ERR_INVALID, "bad label / raw dtype");
    if (lag < 1 || n_items < 0) return fail(ctx, EXABM4D_ERR_INVALID, "lag must be >= 1, n_items >= 0");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    for (int i = 0; i < n_items; i++)
        if (item_patch_host[i] < 0 || item_patch_host[i] >= batch)
            return fail(ctx, EXABM4D_ERR_INVALID, "item patch index out of range");
    for (int i = 0; i < n_items; i++)
        if (item_key_host[i] == 0)   // the kernels' key of every background voxel
            return fail(ctx, EXABM4D_ERR_INVALID, "item key 0 is the background, not a segment");
    if (n_items == 0) return EXABM4D_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = (size_t)n_items * SEG_STATS_K * sizeof(double);
    struct { int32_t* patch; unsigned long long* key; double* out; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.patch = c.take<int32_t>((size_t)n_items * 4);
            r.key = c.take<unsigned long long>((size_t)n_items * 8);
            r.out = c.take<double>(ob);
        }))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(L.patch, item_patch_host, (size_t)n_items * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(L.key, item_key_host, (size_t)n_items * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_segment_stats(labels, label_dtype, raw, raw_dtype, smooth, nz, ny, nx, lag, L.patch, L.key,
                                      n_items, L.out, ctx->stream));
    return fetch(ctx, out_host, L.out, ob);
}

// ---- validation scoring ---------------------------------------------------------------
static_assert(VAL_K == EXABM4D_EVAL_K && VAL_MED == EXABM4D_EVAL_MED && VAL_TARGET_NAN == EXABM4D_EVAL_TARGET_NAN,
              "exabm4d.h and exabm4d_kernels.h differ");

int exabm4d_evaluate_batch_dev(exabm4d_ctx* ctx, const void* pred, int pred_dtype, const void* raw, int raw_dtype,
                               const void* target, int target_dtype, const uint8_t* mask, int batch, size_t n,
                               double k, const uint32_t* ranks, double* out_host) {
    if (!ctx || !pred || !raw || !target || !mask || !ranks || !out_host)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    for (int d : {pred_dtype, raw_dtype, target_dtype})
        if (d != EXABM4D_DT_U16 && d != EXABM4D_DT_F32)
            return fail(ctx, EXABM4D_ERR_INVALID, "pred, raw and target must be uint16 or float32");
    if (batch < 1 || n < 1) return fail(ctx, EXABM4D_ERR_INVALID, "bad batch / sizes");
    if (n >= ((size_t)1 << 32) || batch > EXABM4D_EVAL_MAX_BATCH || n * (size_t)batch > ((size_t)1 << 40))
        return fail(ctx, EXABM4D_ERR_INVALID, "patch or batch too large");
    if (ranks[0] > ranks[1] || ranks[1] - ranks[0] > 1 || ranks[2] > ranks[3] || ranks[1] >= n || ranks[3] >= n)
        return fail(ctx, EXABM4D_ERR_INVALID, "ranks must be two ascending pairs below n, the first one adjacent");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ob = (size_t)batch * VAL_K * sizeof(double);
    struct { double *rows, *partials; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.rows = c.take<double>(ob);
            r.partials = c.take<double>(validate_partials_bytes(batch, n));
        }))
        return rc;
    const ValRanks rk{{ranks[0], ranks[1], ranks[2], ranks[3]}};
    HIP_TRY(ctx, launch_validate_batch(pred, pred_dtype, raw, raw_dtype, target, target_dtype, mask, batch, n, k, rk,
                                       L.partials, L.rows, ctx->stream));
    return fetch(ctx, out_host, L.rows, ob);
}


}  // extern "C"
