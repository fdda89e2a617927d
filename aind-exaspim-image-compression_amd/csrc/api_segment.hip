// api_segment.hip -- the components of a whole volume from those of its bricks' windows: the records a merge needs and
// the relabelled brick.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

namespace {

// The geometry both entries share behind box_geometry(): the window inside the volume, fewer than 2^31 voxels of it.
int segment_geometry(exabm4d_ctx* ctx, const char* who, const int32_t* vol, const int32_t* w0, const int32_t* wd,
                     const int32_t* b0, const int32_t* bd, SegGeom& g) {
    BoxGeom b;
    if (int rc = box_geometry(ctx, who, vol, w0, wd, b0, bd, b)) return rc;
    const std::string name(who);
    g.voxels = g.brick_voxels = 1;
    for (int a = 0; a < 3; a++) {
        g.n[a] = b.n[a];
        g.w0[a] = b.w0[a];
        g.wd[a] = b.wd[a];
        g.b0[a] = b.b0[a];
        g.bd[a] = b.bd[a];
        if ((long long)b.w0[a] + b.wd[a] > b.n[a])
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": the window does not lie inside the volume");
        if (g.voxels > (1ll << 31) / b.wd[a]) return fail(ctx, EXABM4D_ERR_INVALID, name + ": 2^31 labelled voxels or more");
        g.voxels *= b.wd[a];
        g.brick_voxels *= b.bd[a];
    }
    if (g.voxels >= (1ll << 31)) return fail(ctx, EXABM4D_ERR_INVALID, name + ": 2^31 labelled voxels or more");
    return EXABM4D_OK;
}

}  // namespace

extern "C" {

int exabm4d_segment_collect_dev(exabm4d_ctx* ctx, const uint32_t* labels, const int32_t* vol_dims_zyx,
                                const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                const int32_t* brick_origin_zyx, const int32_t* brick_dims_zyx, uint32_t* own,
                                uint64_t* halo, size_t halo_capacity, uint64_t* face, size_t face_capacity,
                                uint64_t* size, size_t size_capacity, uint64_t* counts_dev) {
    if (!ctx || !labels || !own || !halo || !face || !size || !counts_dev)
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (((uintptr_t)labels & 3u) || ((uintptr_t)own & 3u) || ((uintptr_t)halo & 15u) || ((uintptr_t)face & 15u) ||
        ((uintptr_t)size & 15u) || ((uintptr_t)counts_dev & 7u))
        return fail(ctx, EXABM4D_ERR_INVALID, "segment_collect: a misaligned pointer");
    SegGeom g;
    if (int rc = segment_geometry(ctx, "segment_collect", vol_dims_zyx, win_origin_zyx, win_dims_zyx, brick_origin_zyx,
                                  brick_dims_zyx, g))
        return rc;
    if ((long long)halo_capacity < segment_halo_records(g) || (long long)face_capacity < segment_face_records(g))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    "segment_collect: halo_capacity or face_capacity is below the geometric worst case");
    if (size_capacity < 1) return fail(ctx, EXABM4D_ERR_INVALID, "segment_collect: size_capacity must be >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(own, 0, (size_t)g.voxels * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 3 * sizeof(uint64_t), ctx->stream));
    HIP_TRY(ctx, launch_segment_collect(labels, g, own, reinterpret_cast<unsigned long long*>(halo), halo_capacity,
                                        reinterpret_cast<unsigned long long*>(face), face_capacity,
                                        reinterpret_cast<unsigned long long*>(size), size_capacity,
                                        reinterpret_cast<unsigned long long*>(counts_dev), ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_segment_relabel_dev(exabm4d_ctx* ctx, const uint32_t* labels, const int32_t* vol_dims_zyx,
                                const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                const int32_t* brick_origin_zyx, const int32_t* brick_dims_zyx, const uint64_t* keys,
                                const uint64_t* vals, size_t n_keys, int typesize, void* final, void* out) {
    if (!ctx || !labels || !final || !out || (n_keys && (!keys || !vals)))
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (typesize != 4 && typesize != 8) return fail(ctx, EXABM4D_ERR_INVALID, "segment_relabel: typesize must be 4 or 8");
    if (((uintptr_t)labels & 3u) || ((uintptr_t)keys & 7u) || ((uintptr_t)vals & 7u) ||
        ((uintptr_t)final & (uintptr_t)(typesize - 1)) || ((uintptr_t)out & (uintptr_t)(typesize - 1)))
        return fail(ctx, EXABM4D_ERR_INVALID, "segment_relabel: a misaligned pointer");
    SegGeom g;
    if (int rc = segment_geometry(ctx, "segment_relabel", vol_dims_zyx, win_origin_zyx, win_dims_zyx, brick_origin_zyx,
                                  brick_dims_zyx, g))
        return rc;
    if (typesize == 4 && (long long)g.n[0] * g.n[1] * g.n[2] > 0xFFFFFFFFll)
        return fail(ctx, EXABM4D_ERR_INVALID, "segment_relabel: typesize 4 takes a volume of at most 2^32 - 1 voxels");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_segment_relabel(labels, g, reinterpret_cast<const unsigned long long*>(keys),
                                        reinterpret_cast<const unsigned long long*>(vals), n_keys, typesize, final,
                                        out, ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
