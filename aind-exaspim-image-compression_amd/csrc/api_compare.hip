// api_compare.hip -- scoring a box inside a window: the signed difference table, the maximum projections and the
// SSIM sum of a box.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(DIFF_BINS == EXABM4D_DIFF_BINS, "exabm4d.h and exabm4d_kernels.h differ");

// scipy's "reflect" of an index into [0, n): what reflect_idx of metrics_kernels.hip computes
static int reflect_host(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

extern "C" {

int exabm4d_diff_histogram_u16_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                                   const uint16_t* mask_win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int zero_first,
                                   uint64_t* hist_dev) {
    if (!ctx || !ref_win || !test_win || !hist_dev) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    BoxGeom g;
    if (int rc = box_geometry(ctx, "diff_histogram_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx,
                              box_dims_zyx, g))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (zero_first)
        HIP_TRY(ctx, hipMemsetAsync(hist_dev, 0, (size_t)(mask_win ? 2 : 1) * DIFF_BINS * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, launch_diff_hist_u16(ref_win, test_win, mask_win, g, reinterpret_cast<unsigned long long*>(hist_dev),
                                      ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_mip3_u16_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                         const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                         const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, uint32_t* planes_dev) {
    if (!ctx || !ref_win || !test_win || !planes_dev) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    BoxGeom g;
    if (int rc = box_geometry(ctx, "mip3_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx, box_dims_zyx, g))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_mip3_u16(ref_win, test_win, g, planes_dev, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_ssim3d_box_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                           const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                           const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int window, double c1,
                           double c2, double* sum_host) {
    if (!ctx || !ref_win || !test_win || !sum_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    BoxGeom g;
    if (int rc = box_geometry(ctx, "ssim3d_box", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx, box_dims_zyx, g))
        return rc;
    if (window < 1 || window > ssim3d_max_window())
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED, "ssim window must be 1..32");
    // every sample the box's voxels read, per axis: the kernel reads reflect(i, n) - w0 for exactly these i
    const int left = window / 2;
    for (int a = 0; a < 3; a++) {
        if (g.n[a] < window && (g.w0[a] != 0 || g.wd[a] != g.n[a]))
            return fail(ctx, EXABM4D_ERR_INVALID, "ssim3d_box: an axis shorter than the ssim window must be in the window whole");
        for (int i = g.b0[a] - left; i <= g.b0[a] + g.bd[a] - 1 + window - left - 1; i++) {
            const int r = reflect_host(i, g.n[a]);
            if (r < g.w0[a] || r >= g.w0[a] + g.wd[a])
                return fail(ctx, EXABM4D_ERR_INVALID, "ssim3d_box: the window does not cover the box and its ssim halo");
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)ssim3d_partials(g.bd[0], g.bd[1], g.bd[2]);
    if (int rc = grow(ctx, ctx->red, (np + 1) * sizeof(double))) return rc;
    double* d = ctx->red.as<double>();
    HIP_TRY(ctx, launch_ssim3d_box(ref_win, test_win, g, window, c1, c2, d + 1, d, ctx->stream));
    return fetch(ctx, sum_host, d, sizeof(double));
}

}  // extern "C"
