// api_foreground.hip -- the foreground mask of a box inside a window, and the uint16 -> byte mask
// conversion of re-coding a store under a mask store.  Host code only; the context and the shared helpers are in
// exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(FG_MAX_RADIUS == EXABM4D_FG_MAX_RADIUS, "exabm4d.h and exabm4d_kernels.h differ");

extern "C" {

int exabm4d_foreground_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int cut, int radius,
                                   int value, uint16_t* out_u16, uint8_t* out_u8, uint64_t* counts_dev,
                                   int zero_first) {
    if (!ctx || !win) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!out_u16 && !out_u8) return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: out_u16 and out_u8 are both NULL");
    if (cut < 0 || cut > 65536) return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: cut must be 0..65536");
    if (radius < 0 || radius > EXABM4D_FG_MAX_RADIUS)
        return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: radius must be 0..EXABM4D_FG_MAX_RADIUS");
    if (value < 1 || value > 65535) return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: value must be 1..65535");
    if (((uintptr_t)win & 1u) || ((uintptr_t)out_u16 & 1u) || ((uintptr_t)counts_dev & 7u))
        return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: a misaligned pointer");
    BoxGeom g;
    if (int rc = box_geometry(ctx, "foreground_box_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx,
                              box_dims_zyx, g))
        return rc;
    for (int a = 0; a < 3; a++) {
        const int lo = std::max(0, g.b0[a] - radius), hi = std::min(g.n[a], g.b0[a] + g.bd[a] + radius);
        if (lo < g.w0[a] || hi > g.w0[a] + g.wd[a])
            return fail(ctx, EXABM4D_ERR_INVALID,
                        "foreground_box_u16: the window does not hold the box grown by the radius (cut at the volume)");
    }
    FgPlan plan;
    if (!foreground_box_plan(win, g, radius, out_u16, out_u8, plan))
        return fail(ctx, EXABM4D_ERR_INVALID, "foreground_box_u16: the box is too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->foreground_ready) {
        HIP_TRY(ctx, foreground_prepare());
        ctx->foreground_ready = 1;
    }
    if (counts_dev && zero_first) HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 2 * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, launch_foreground_box_u16(win, g, plan, (uint32_t)cut, radius, (uint32_t)value, out_u16, out_u8,
                                           reinterpret_cast<unsigned long long*>(counts_dev), ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_nonzero_u8_dev(exabm4d_ctx* ctx, const uint16_t* src, size_t n, uint8_t* dst) {
    if (!ctx || (n && (!src || !dst))) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((uintptr_t)src & 1u) return fail(ctx, EXABM4D_ERR_INVALID, "nonzero_u8: src at an odd address");
    if (n > ((size_t)1 << 40)) return fail(ctx, EXABM4D_ERR_INVALID, "nonzero_u8: too many elements");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_nonzero_u8(src, dst, n, ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
