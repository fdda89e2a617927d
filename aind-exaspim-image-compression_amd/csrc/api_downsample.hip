// api_downsample.hip -- one pyramid level of a box inside a window: uint16 counts and uint32 / uint64
// labels (5.24).  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(DS_MODE == EXABM4D_DS_MODE && DS_MEAN == EXABM4D_DS_MEAN && DS_MAX == EXABM4D_DS_MAX &&
                  DS_CROP == EXABM4D_DS_CROP && DS_PARTIAL == EXABM4D_DS_PARTIAL &&
                  LABEL_ZEROS_COUNT == EXABM4D_LABEL_ZEROS_COUNT && LABEL_ZEROS_IGNORE == EXABM4D_LABEL_ZEROS_IGNORE,
              "exabm4d.h and exabm4d_kernels.h differ");

// The checks both entries make of the factors and the three boxes, in one order; fills g.  EXABM4D_OK or the failure.
static int downsample_geometry(exabm4d_ctx* ctx, const char* who, const int32_t* vol_dims_zyx,
                               const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                               const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, const int32_t* factors_zyx,
                               int edge, BoxGeom& g) {
    int product = 1;
    for (int a = 0; a < 3; a++) {
        if (factors_zyx[a] != 1 && factors_zyx[a] != 2)
            return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": every factor must be 1 or 2");
        product *= factors_zyx[a];
    }
    if (product == 1) return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": one factor at least must be 2");
    long long voxels = 1;
    for (int a = 0; a < 3; a++) {
        const int f = factors_zyx[a];
        g.n[a] = vol_dims_zyx[a];
        g.w0[a] = win_origin_zyx[a];
        g.wd[a] = win_dims_zyx[a];
        g.b0[a] = box_origin_zyx[a];
        g.bd[a] = box_dims_zyx[a];
        if (g.n[a] < 1 || g.wd[a] < 1 || g.bd[a] < 1)
            return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": every extent must be >= 1");
        if (g.n[a] > (1 << 20)) return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": volume too large");
        voxels *= g.n[a];
        // a window may run past the volume's upper faces (a reader's padding): nothing there enters a result
        if (g.w0[a] < 0 || g.w0[a] >= g.n[a] || g.wd[a] > (1 << 21))
            return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": the window does not begin inside the volume");
        const int level = edge == DS_CROP ? g.n[a] / f : (g.n[a] + f - 1) / f;
        if (g.b0[a] < 0 || (long long)g.b0[a] + g.bd[a] > level)
            return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": the box does not lie inside the level");
        const long long lo = (long long)g.b0[a] * f;
        const long long hi = std::min<long long>(g.n[a], ((long long)g.b0[a] + g.bd[a]) * f);
        if (lo < g.w0[a] || hi > (long long)g.w0[a] + g.wd[a])
            return fail(ctx, EXABM4D_ERR_INVALID,
                        std::string(who) + ": the window does not hold the box's source voxels (cut at the volume)");
    }
    if (voxels > (1ll << 40)) return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": volume too large");
    return EXABM4D_OK;
}

extern "C" {

int exabm4d_downsample_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                   const int32_t* factors_zyx, int method, int edge, uint16_t* out_u16) {
    if (!ctx || !win || !out_u16 || !vol_dims_zyx || !win_origin_zyx || !win_dims_zyx || !box_origin_zyx ||
        !box_dims_zyx || !factors_zyx)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (((uintptr_t)win & 1u) || ((uintptr_t)out_u16 & 1u))
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_u16: a misaligned pointer");
    if (method != DS_MODE && method != DS_MEAN && method != DS_MAX)
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_u16: method must be EXABM4D_DS_MODE, _MEAN or _MAX");
    if (edge != DS_CROP && edge != DS_PARTIAL)
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_u16: edge must be EXABM4D_DS_CROP or _PARTIAL");
    BoxGeom g;
    const int rc = downsample_geometry(ctx, "downsample_box_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx,
                                       box_origin_zyx, box_dims_zyx, factors_zyx, edge, g);
    if (rc != EXABM4D_OK) return rc;
    DsPlan plan;
    const int factors[3] = {factors_zyx[0], factors_zyx[1], factors_zyx[2]};
    downsample_box_plan(win, g, factors, out_u16, plan);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_downsample_box_u16(win, g, plan, method, out_u16, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_downsample_box_labels_dev(exabm4d_ctx* ctx, const void* win, int typesize, const int32_t* vol_dims_zyx,
                                      const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                      const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                      const int32_t* factors_zyx, int edge, int zeros, void* out) {
    if (!ctx || !win || !out || !vol_dims_zyx || !win_origin_zyx || !win_dims_zyx || !box_origin_zyx ||
        !box_dims_zyx || !factors_zyx)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((typesize == 4 || typesize == 8) &&
        (((uintptr_t)win & (uintptr_t)(typesize - 1)) || ((uintptr_t)out & (uintptr_t)(typesize - 1))))
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_labels: a misaligned pointer");
    if (typesize != 4 && typesize != 8)
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_labels: typesize must be 4 or 8");
    if (edge != DS_CROP && edge != DS_PARTIAL)
        return fail(ctx, EXABM4D_ERR_INVALID, "downsample_box_labels: edge must be EXABM4D_DS_CROP or _PARTIAL");
    if (zeros != LABEL_ZEROS_COUNT && zeros != LABEL_ZEROS_IGNORE)
        return fail(ctx, EXABM4D_ERR_INVALID,
                    "downsample_box_labels: zeros must be EXABM4D_LABEL_ZEROS_COUNT or _IGNORE");
    BoxGeom g;
    const int rc = downsample_geometry(ctx, "downsample_box_labels", vol_dims_zyx, win_origin_zyx, win_dims_zyx,
                                       box_origin_zyx, box_dims_zyx, factors_zyx, edge, g);
    if (rc != EXABM4D_OK) return rc;
    DsPlan plan;
    const int factors[3] = {factors_zyx[0], factors_zyx[1], factors_zyx[2]};
    label_downsample_box_plan(win, typesize, g, factors, out, plan);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_downsample_box_labels(win, typesize, g, plan, zeros, out, ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
