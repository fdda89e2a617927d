// api_components.hip -- the connected components of the seeds of a window, their sizes and the filter by size
// (DESIGN.md 5.20).  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(CC_TZ == EXABM4D_CC_TILE_Z && CC_TY == EXABM4D_CC_TILE_Y && CC_TX == EXABM4D_CC_TILE_X,
              "exabm4d.h and exabm4d_kernels.h differ");

namespace {

// What both entries share behind their own checks: the region, the scratch, the launches.
int run_components(exabm4d_ctx* ctx, const char* who, const void* win, bool win_u8, const BoxGeom& b,
                   const int32_t* count0, const int32_t* countd, int cut, int min_voxels, int connectivity,
                   uint16_t* out16, uint8_t* out8, uint32_t* labels, uint32_t* sizes, void* scratch,
                   size_t scratch_bytes, uint64_t* counts_dev, int zero_first) {
    const std::string name(who);
    if (connectivity != 6 && connectivity != 26)
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": connectivity must be 6 or 26");
    if (min_voxels < 1) return fail(ctx, EXABM4D_ERR_INVALID, name + ": min_voxels must be >= 1");
    if (cut < 0 || cut > 65536) return fail(ctx, EXABM4D_ERR_INVALID, name + ": cut must be 0..65536");
    if (!scratch) return fail(ctx, EXABM4D_ERR_INVALID, name + ": NULL scratch");
    if (((uintptr_t)scratch & 3u) || ((uintptr_t)labels & 3u) || ((uintptr_t)sizes & 3u) ||
        ((uintptr_t)out16 & 1u) || ((uintptr_t)counts_dev & 7u))
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": a misaligned pointer");
    for (int a = 0; a < 3; a++)
        if (countd[a] < 0 || count0[a] < b.b0[a] || (long long)count0[a] + countd[a] > (long long)b.b0[a] + b.bd[a])
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": the count box does not lie inside the box");
    CcGeom g;
    if (!components_geometry(b, count0, countd, min_voxels - 1, g))
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": 2^31 labelled voxels or more");
    for (int a = 0; a < 3; a++)
        if (g.r0[a] < b.w0[a] || g.r0[a] + g.rd[a] > b.w0[a] + b.wd[a])
            return fail(ctx, EXABM4D_ERR_INVALID,
                        name + ": the window does not hold the box grown by min_voxels - 1 (cut at the volume)");
    if (scratch_bytes < components_scratch_bytes(g.voxels))
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": scratch_bytes is less than the labelled region takes");
    const size_t each = components_scratch_bytes(g.voxels) / 3;
    uint32_t* parent = static_cast<uint32_t*>(scratch);
    if (!labels) labels = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + each);
    if (!sizes) sizes = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + 2 * each);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (counts_dev && zero_first) HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 3 * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, launch_components(win, win_u8, g, (uint32_t)cut, (uint32_t)min_voxels, connectivity, parent, labels,
                                   sizes, out16, out8, reinterpret_cast<unsigned long long*>(counts_dev),
                                   ctx->stream));
    return EXABM4D_OK;
}

}  // namespace

extern "C" {

size_t exabm4d_components_scratch_bytes(const int32_t* win_dims_zyx, int connectivity) {
    if (!win_dims_zyx || (connectivity != 6 && connectivity != 26)) return 0;
    long long voxels = 1;
    for (int a = 0; a < 3; a++) {
        if (win_dims_zyx[a] < 1 || voxels > (1ll << 31) / win_dims_zyx[a]) return 0;
        voxels *= win_dims_zyx[a];
    }
    return voxels < (1ll << 31) ? components_scratch_bytes(voxels) : 0;
}

int exabm4d_component_seeds_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                    const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                    const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                    const int32_t* count_origin_zyx, const int32_t* count_dims_zyx, int cut,
                                    int min_voxels, int connectivity, uint16_t* seeds_u16, uint32_t* labels,
                                    uint32_t* sizes, void* scratch, size_t scratch_bytes, uint64_t* counts_dev,
                                    int zero_first) {
    if (!ctx || !win || !count_origin_zyx || !count_dims_zyx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((uintptr_t)win & 1u) return fail(ctx, EXABM4D_ERR_INVALID, "component_seeds_u16: a misaligned pointer");
    BoxGeom b;
    if (int rc = box_geometry(ctx, "component_seeds_u16", vol_dims_zyx, win_origin_zyx, win_dims_zyx, box_origin_zyx,
                              box_dims_zyx, b))
        return rc;
    return run_components(ctx, "component_seeds_u16", win, false, b, count_origin_zyx, count_dims_zyx, cut, min_voxels,
                          connectivity, seeds_u16, nullptr, labels, sizes, scratch, scratch_bytes, counts_dev,
                          zero_first);
}

int exabm4d_label_components_dev(exabm4d_ctx* ctx, const void* src, int src_u16, const int32_t* dims_zyx, int cut,
                                 int min_voxels, int connectivity, uint32_t* labels, uint32_t* sizes,
                                 uint8_t* kept_u8, void* scratch, size_t scratch_bytes, uint64_t* counts_dev) {
    if (!ctx || !src || !dims_zyx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (src_u16 && ((uintptr_t)src & 1u))
        return fail(ctx, EXABM4D_ERR_INVALID, "label_components: a misaligned pointer");
    const int32_t zero[3] = {0, 0, 0};
    BoxGeom b;
    if (int rc = box_geometry(ctx, "label_components", dims_zyx, zero, dims_zyx, zero, dims_zyx, b)) return rc;
    return run_components(ctx, "label_components", src, !src_u16, b, zero, dims_zyx, src_u16 ? cut : 1, min_voxels,
                          connectivity, nullptr, kept_u8, labels, sizes, scratch, scratch_bytes, counts_dev, 1);
}

}  // extern "C"
