// api_sampler.hip -- the patch samplers' device entries: foreground counts without a mask and the
// annotation masks of a batch of boxes.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(RASTER_BOXES == EXABM4D_RASTER_BOXES, "exabm4d.h and exabm4d_kernels.h differ");

extern "C" {

int exabm4d_foreground_counts_dev(exabm4d_ctx* ctx, const void* raw, int dtype, int batch, int nz, int ny, int nx,
                                  float k, int dilate, uint32_t* counts_host, float* thr_host) {
    if (!ctx || !raw || !counts_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (dtype != EXABM4D_DT_U16 && dtype != EXABM4D_DT_F32)
        return fail(ctx, EXABM4D_ERR_INVALID, "raw must be uint16 or float32");
    if (dilate < 0) return fail(ctx, EXABM4D_ERR_INVALID, "dilate must be >= 0");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    if (count_workgroups(batch, nz, ny, nx) >= (1ll << 31)) return fail(ctx, EXABM4D_ERR_INVALID, "batch too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)nz * ny * nx * batch;
    struct { float* thr; uint32_t* counts; uint8_t *mask, *tmp; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.thr = c.take<float>((size_t)batch * sizeof(float));
            r.counts = c.take<uint32_t>((size_t)batch * sizeof(uint32_t));
            r.mask = c.take<uint8_t>(dilate > 1 ? total : 0);
            r.tmp = c.take<uint8_t>(dilate > 2 ? total : 0);
        }))
        return rc;
    HIP_TRY(ctx, launch_fg_threshold(raw, dtype, batch, (size_t)nz * ny * nx, k, L.thr, ctx->stream));
    if (dilate <= 1) {
        HIP_TRY(ctx, launch_count_above(raw, dtype, L.thr, batch, nz, ny, nx, dilate, L.counts, ctx->stream));
    } else {   // all but the last dilation through the mask path; the count kernel makes the last one
        HIP_TRY(ctx, launch_dilate(nullptr, raw, dtype, L.thr, batch, nz, ny, nx, dilate - 1, L.tmp, L.mask,
                                   ctx->stream));
        HIP_TRY(ctx, launch_count_mask(L.mask, batch, nz, ny, nx, 1, L.counts, ctx->stream));
    }
    if (thr_host)
        HIP_TRY(ctx, hipMemcpyAsync(thr_host, L.thr, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost,
                                    ctx->stream));
    return fetch(ctx, counts_host, L.counts, (size_t)batch * sizeof(uint32_t));
}

int exabm4d_annotation_masks_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, int seg_dilate,
                                 const int32_t* points, size_t npoints, const int32_t* starts_host, int skel_dilate,
                                 int batch, int nz, int ny, int nx, uint8_t* mask) {
    if (!ctx || !mask) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!labels && !points) return fail(ctx, EXABM4D_ERR_INVALID, "neither labels nor points: no annotation");
    if (labels && bad_label_dtype(label_dtype)) return fail(ctx, EXABM4D_ERR_INVALID, "bad label dtype");
    if (points && !starts_host) return fail(ctx, EXABM4D_ERR_INVALID, "points need the box origins");
    if (seg_dilate < 0 || skel_dilate < 0) return fail(ctx, EXABM4D_ERR_INVALID, "dilations must be >= 0");
    if (npoints > ((size_t)1 << 40)) return fail(ctx, EXABM4D_ERR_INVALID, "too many points");
    if (int rc = check_patches(ctx, batch, nz, ny, nx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)nz * ny * nx, total = n * batch;
    // raster: the points' own mask when it must be dilated; skel: its dilation when labels hold `mask` already
    const bool dil = points && skel_dilate > 0;
    const int most = seg_dilate > skel_dilate ? seg_dilate : skel_dilate;
    struct { int32_t* starts; uint8_t *raster, *skel, *tmp; } L;
    if (int rc = carve(ctx, ctx->red, 0, L, [&](Carver& c, auto& r) {
            r.starts = c.take<int32_t>(points ? (size_t)batch * 3 * sizeof(int32_t) : 0);
            r.raster = c.take<uint8_t>(dil ? total : 0);
            r.skel = c.take<uint8_t>(dil && labels ? total : 0);
            r.tmp = c.take<uint8_t>(most > 1 ? total : 0);
        }))
        return rc;
    if (labels)
        HIP_TRY(ctx, launch_dilate_labels(labels, label_dtype, batch, nz, ny, nx, seg_dilate, L.tmp, mask,
                                          ctx->stream));
    if (points) {
        // undilated points go straight into `mask`: a store of 1 is the OR with what the labels left there
        uint8_t* dst = dil ? L.raster : mask;
        if (dil || !labels) HIP_TRY(ctx, hipMemsetAsync(dst, 0, total, ctx->stream));
        if (npoints) {
            HIP_TRY(ctx, hipMemcpyAsync(L.starts, starts_host, (size_t)batch * 3 * sizeof(int32_t),
                                        hipMemcpyHostToDevice, ctx->stream));
            for (int b0 = 0; b0 < batch; b0 += RASTER_BOXES) {
                const int nb = batch - b0 < RASTER_BOXES ? batch - b0 : RASTER_BOXES;
                const int ext[3] = {nz, ny, nx};
                RasterBounds bb;
                for (int a = 0; a < 3; a++) {
                    bb.lo[a] = bb.hi[a] = starts_host[3 * b0 + a];
                    for (int b = b0; b < b0 + nb; b++) {
                        const long long s = starts_host[3 * b + a];
                        bb.lo[a] = s < bb.lo[a] ? s : bb.lo[a];
                        bb.hi[a] = s > bb.hi[a] ? s : bb.hi[a];
                    }
                    bb.hi[a] += ext[a];
                }
                HIP_TRY(ctx, launch_raster_points(points, npoints, L.starts + 3 * (size_t)b0, nb, nz, ny, nx, bb,
                                                  dst + (size_t)b0 * n, ctx->stream));
            }
        }
        if (dil) {
            uint8_t* out = labels ? L.skel : mask;
            HIP_TRY(ctx, launch_dilate(L.raster, nullptr, 0, nullptr, batch, nz, ny, nx, skel_dilate, L.tmp, out,
                                       ctx->stream));
            if (labels) HIP_TRY(ctx, launch_or_bytes(L.skel, total, mask, ctx->stream));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // also: starts_host has been read
    return EXABM4D_OK;
}

}  // extern "C"
