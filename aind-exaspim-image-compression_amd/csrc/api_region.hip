// api_region.hip -- region reads of a chunk store: boxes gathered from a pool of decoded chunks.
// Host code only; the context and the shared helpers are in exabm4d_api.h.
#include <cstddef>

#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(sizeof(BoxSrc) == sizeof(exabm4d_box_src) && offsetof(BoxSrc, stride_z) == offsetof(exabm4d_box_src, stride_z) &&
              offsetof(BoxSrc, z0) == offsetof(exabm4d_box_src, z0) && offsetof(BoxSrc, ex) == offsetof(exabm4d_box_src, ex),
              "exabm4d.h and exabm4d_kernels.h differ");

// Does the source lie inside [0, pool_elems)?  Its last element is base + (ez-1) stride_z + (ey-1) stride_y + (ex-1);
// every term is bounded by pool_elems before it is used, so nothing overflows.
static bool source_inside(const exabm4d_box_src& s, size_t pool_elems) {
    auto add = [&](uint64_t& at, uint64_t count, uint64_t step) {      // at += count * step, false past the pool
        if (count == 0) return true;
        if (step > pool_elems || count > pool_elems) return false;
        const unsigned __int128 t = (unsigned __int128)count * step + at;
        if (t >= pool_elems) return false;
        at = (uint64_t)t;
        return true;
    };
    uint64_t at = s.base;
    if (at >= pool_elems) return false;
    return add(at, (uint64_t)(s.ez - 1), s.stride_z) && add(at, (uint64_t)(s.ey - 1), s.stride_y) &&
           add(at, (uint64_t)(s.ex - 1), 1);
}

extern "C" {

int exabm4d_gather_boxes_dev(exabm4d_ctx* ctx, const uint16_t* pool, size_t pool_elems,
                             const exabm4d_box_src* srcs_host, int nsrc, const int32_t* box_srcs_host, int per_box,
                             const int32_t* starts_host, int nbox, int bz, int by, int bx, int out_dtype,
                             float offset, double fill, void* out) {
    if (!ctx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (out_dtype != EXABM4D_DT_U16 && out_dtype != EXABM4D_DT_F32)
        return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: out must be uint16 or float32");
    if (nbox < 0 || nsrc < 0 || per_box < 0 || bz < 1 || by < 1 || bx < 1)
        return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: bad sizes");
    if ((unsigned long long)bz * by >= (1ull << 31) || (unsigned long long)bz * by * bx > (1ull << 40) ||
        (unsigned long long)bz * by * bx * (unsigned long long)nbox > (1ull << 40) ||
        (unsigned long long)nbox * (unsigned long long)per_box > (1ull << 31))
        return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: boxes, batch or source lists too large");
    const bool f32 = out_dtype == EXABM4D_DT_F32;
    if (!f32 && !(fill >= 0.0 && fill <= 65535.0 && fill == std::floor(fill)))
        return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: a uint16 fill must be an integer in 0..65535");
    if (nbox == 0) return EXABM4D_OK;
    if (!out || !starts_host || (nsrc && (!pool || !srcs_host)) || (per_box && !box_srcs_host))
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    const size_t esz = f32 ? 4 : 2;
    if (((uintptr_t)pool & 1) || ((uintptr_t)out & (esz - 1)))
        return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: pool or out below the natural alignment of its elements");
    for (int i = 0; i < nsrc; i++) {
        const exabm4d_box_src& s = srcs_host[i];
        if (s.ez < 1 || s.ey < 1 || s.ex < 1) return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: a source extent below 1");
        if (!source_inside(s, pool_elems))
            return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: a source reaches outside the pool");
    }
    const size_t nlist = (size_t)nbox * per_box;
    for (size_t i = 0; i < nlist; i++)
        if (box_srcs_host[i] < -1 || box_srcs_host[i] >= nsrc)
            return fail(ctx, EXABM4D_ERR_INVALID, "gather_boxes: a source list entry outside [-1, nsrc)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // one pinned image of the three tables, one copy
    struct Tables { BoxSrc* srcs; int32_t *lists, *starts; };
    auto layout = [&](Carver& c, Tables& r) {
        r.srcs = c.take<BoxSrc>((size_t)nsrc * sizeof(BoxSrc));
        r.lists = c.take<int32_t>(nlist * 4);
        r.starts = c.take<int32_t>((size_t)nbox * 12);
    };
    Tables L, H;                                    // on the device, in the pinned image
    if (int rc = carve(ctx, ctx->region_tab, 0, L, layout)) return rc;
    Carver sized;
    layout(sized, H);                               // a pass without a base only adds up the bytes
    const size_t bytes = sized.at;
    if (!ctx->region_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->region_ev, hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(ctx->region_ev));       // the last copy out of the pinned image is done
    if (bytes > ctx->region_host_bytes) {
        if (ctx->region_host) (void)hipHostFree(ctx->region_host);
        ctx->region_host = nullptr;
        ctx->region_host_bytes = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->region_host, bytes, hipHostMallocDefault));
        ctx->region_host_bytes = bytes;
    }
    char* dev0 = ctx->region_tab.as<char>();
    Carver h{static_cast<char*>(ctx->region_host)};
    layout(h, H);
    if (nsrc) std::memcpy(H.srcs, srcs_host, (size_t)nsrc * sizeof(BoxSrc));
    if (nlist) std::memcpy(H.lists, box_srcs_host, nlist * 4);
    std::memcpy(H.starts, starts_host, (size_t)nbox * 12);
    HIP_TRY(ctx, hipMemcpyAsync(dev0, ctx->region_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->region_ev, ctx->stream));
    HIP_TRY(ctx, launch_gather_boxes(pool, L.srcs, L.lists, per_box, L.starts, nbox, bz, by, bx, f32 ? 1 : 0, offset,
                                     (float)fill, f32 ? (uint16_t)0 : (uint16_t)fill, out, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_scatter_boxes_dev(exabm4d_ctx* ctx, const void* src, size_t src_elems, int src_dtype,
                              const exabm4d_box_src* boxes_host, int nbox, void* pool, size_t pool_elems,
                              int pool_dtype, const exabm4d_box_src* dsts_host, int ndst,
                              const int32_t* dst_boxes_host, int per_dst, float offset) {
    if (!ctx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    int kind;
    size_t ssz, psz;
    if (src_dtype == EXABM4D_DT_U16 && pool_dtype == EXABM4D_DT_U16) kind = SCATTER_U16, ssz = 2, psz = 2;
    else if (src_dtype == EXABM4D_DT_F32 && pool_dtype == EXABM4D_DT_U16) kind = SCATTER_F32, ssz = 4, psz = 2;
    else if (src_dtype == EXABM4D_DT_U8 && pool_dtype == EXABM4D_DT_U8) kind = SCATTER_U8, ssz = 1, psz = 1;
    else
        return fail(ctx, EXABM4D_ERR_INVALID,
                    "scatter_boxes: (src, pool) must be (uint16, uint16), (float32, uint16) or (uint8, uint8)");
    if (nbox < 0 || ndst < 0 || per_dst < 0) return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: bad sizes");
    if ((unsigned long long)ndst * (unsigned long long)per_dst > (1ull << 31))
        return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: box lists too large");
    if (kind == SCATTER_F32 && !(offset == offset))
        return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: the offset is NaN");
    if ((ndst && !dsts_host) || (nbox && !boxes_host) || (ndst && per_dst && !dst_boxes_host))
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (((uintptr_t)src & (ssz - 1)) || ((uintptr_t)pool & (psz - 1)))
        return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: src or pool below the natural alignment of its elements");
    for (int i = 0; i < nbox; i++) {
        const exabm4d_box_src& b = boxes_host[i];
        if (b.ez < 1 || b.ey < 1 || b.ex < 1) return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a box extent below 1");
        if (!source_inside(b, src_elems))
            return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a box reaches outside src");
    }
    unsigned long long rows = 0;
    for (int i = 0; i < ndst; i++) {
        const exabm4d_box_src& d = dsts_host[i];
        if (d.ez < 1 || d.ey < 1 || d.ex < 1)
            return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a destination extent below 1");
        if ((unsigned long long)d.ez * (unsigned long long)d.ey >= (1ull << 31))
            return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a destination too large");
        if (!source_inside(d, pool_elems))
            return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a destination reaches outside the pool");
        rows += (unsigned long long)d.ez * (unsigned long long)d.ey;
    }
    const size_t nlist = (size_t)ndst * per_dst;
    for (size_t i = 0; i < nlist; i++)
        if (dst_boxes_host[i] < -1 || dst_boxes_host[i] >= nbox)
            return fail(ctx, EXABM4D_ERR_INVALID, "scatter_boxes: a box list entry outside [-1, nbox)");
    if (ndst == 0 || nbox == 0 || per_dst == 0) return EXABM4D_OK;     // no box reaches a destination
    if (!src || !pool) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // one pinned image of the four tables, one copy (the gather's buffers: the event orders their reuse)
    struct Tables { BoxSrc *boxes, *dsts; unsigned long long* row0; int32_t* lists; };
    auto layout = [&](Carver& c, Tables& r) {
        r.boxes = c.take<BoxSrc>((size_t)nbox * sizeof(BoxSrc));
        r.dsts = c.take<BoxSrc>((size_t)ndst * sizeof(BoxSrc));
        r.row0 = c.take<unsigned long long>(((size_t)ndst + 1) * 8);
        r.lists = c.take<int32_t>(nlist * 4);
    };
    Tables L, H;                                    // on the device, in the pinned image
    if (int rc = carve(ctx, ctx->region_tab, 0, L, layout)) return rc;
    Carver sized;
    layout(sized, H);                               // a pass without a base only adds up the bytes
    const size_t bytes = sized.at;
    if (!ctx->region_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->region_ev, hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(ctx->region_ev));       // the last copy out of the pinned image is done
    if (bytes > ctx->region_host_bytes) {
        if (ctx->region_host) (void)hipHostFree(ctx->region_host);
        ctx->region_host = nullptr;
        ctx->region_host_bytes = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->region_host, bytes, hipHostMallocDefault));
        ctx->region_host_bytes = bytes;
    }
    char* dev0 = ctx->region_tab.as<char>();
    Carver h{static_cast<char*>(ctx->region_host)};
    layout(h, H);
    std::memcpy(H.boxes, boxes_host, (size_t)nbox * sizeof(BoxSrc));
    std::memcpy(H.dsts, dsts_host, (size_t)ndst * sizeof(BoxSrc));
    H.row0[0] = 0;
    for (int i = 0; i < ndst; i++)
        H.row0[i + 1] = H.row0[i] + (unsigned long long)dsts_host[i].ez * (unsigned long long)dsts_host[i].ey;
    std::memcpy(H.lists, dst_boxes_host, nlist * 4);
    HIP_TRY(ctx, hipMemcpyAsync(dev0, ctx->region_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->region_ev, ctx->stream));
    HIP_TRY(ctx, launch_scatter_boxes(src, kind, L.boxes, L.dsts, L.row0, ndst, L.lists, per_dst, rows, offset, pool,
                                      ctx->stream));
    return EXABM4D_OK;
}

}  // extern "C"
