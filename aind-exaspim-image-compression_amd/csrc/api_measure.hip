// api_measure.hip -- measuring a box inside a window: the table of the counts and the wide noise table, added to
// tables resident on the device.  Host code only; the context and the shared helpers are in
// exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(COUNT_BINS == EXABM4D_COUNT_BINS && NOISE_WIDE_BINS == EXABM4D_NOISE_WIDE_BINS,
              "exabm4d.h and exabm4d_kernels.h differ");

extern "C" {

int exabm4d_measure_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const uint16_t* mask_win,
                                const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx,
                                const int32_t* win_dims_zyx, const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                int zero_first, uint64_t* counts_dev, uint64_t* noise_dev) {
    if (!ctx || !win || !counts_dev || !noise_dev) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    BoxGeom g;
    if (int rc = box_geometry(ctx, "measure_box_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx,
                              box_dims_zyx, g))
        return rc;
    // The cells the box owns are those with an even origin in the box and below n & ~1, per axis; the far corner of
    // the last of them along an axis is the highest index read there.
    for (int a = 0; a < 3; a++) {
        const int last = std::min(g.b0[a] + g.bd[a] - 1, (g.n[a] & ~1) - 1) & ~1;     // its origin, if there is one
        if (last >= g.b0[a] && last + 1 >= g.w0[a] + g.wd[a])
            return fail(ctx, EXABM4D_ERR_INVALID,
                        "measure_box_u16: the window does not hold the far corner of a cell that begins in the box");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->measure_wgs) HIP_TRY(ctx, measure_prepare(ctx->device, &ctx->measure_wgs));
    MeasurePlan plan;
    if (!measure_box_plan(win, mask_win, g, ctx->measure_wgs, plan))
        return fail(ctx, EXABM4D_ERR_INVALID, "measure_box_u16: the box is too large");
    const int tables = mask_win ? 2 : 1;
    if (zero_first) {
        HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, measure_counts_bytes(tables), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(noise_dev, 0, measure_noise_bytes(tables), ctx->stream));
    }
    HIP_TRY(ctx, launch_measure_box_u16(win, mask_win, g, plan, reinterpret_cast<unsigned long long*>(counts_dev),
                                        reinterpret_cast<unsigned long long*>(noise_dev), ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
