// api_labels.hip -- the label codec `exac-labels`: bound, encode, decode of a volume, and boxes
// gathered straight from coded chunks.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include <cstddef>

#include "exabm4d_api.h"

using namespace exabm4d;

static_assert(sizeof(LabelChunkSrc) == sizeof(exabm4d_label_src) && offsetof(LabelChunkSrc, bytes) == offsetof(exabm4d_label_src, bytes) &&
              offsetof(LabelChunkSrc, z0) == offsetof(exabm4d_label_src, z0) && offsetof(LabelChunkSrc, ex) == offsetof(exabm4d_label_src, ex),
              "exabm4d.h and exabm4d_kernels.h differ");

static const char* const LB_GEOM_RULE =
    "label codec: typesize must be 4 or 8, sizes >= 1, chunk <= 2^27 voxels, volume <= 2^40";

// aux layout: sizes u32[nchunks] | offsets u64[nchunks + 1] | totals u64[2] | status u32[4]
struct LabelAux { uint32_t* sizes; unsigned long long *offsets, *totals; uint32_t* status; };
static int label_aux(exabm4d_ctx* ctx, int nchunks, LabelAux& A) {
    return carve(ctx, ctx->codec_aux, 0, A, [&](Carver& c, auto& r) {
        r.sizes = c.take<uint32_t>((size_t)nchunks * 4);
        r.offsets = c.take<unsigned long long>(((size_t)nchunks + 1) * 8);
        r.totals = c.take<unsigned long long>(2 * 8);
        r.status = c.take<uint32_t>(4 * 4);
    });
}
// The decoders' status word, fetched after the kernel: nonzero is a malformed stream or a palette index >= k.
static int label_status(exabm4d_ctx* ctx, const uint32_t* status, const char* who) {
    uint32_t st = 0;
    if (int rc = fetch(ctx, &st, status, sizeof st)) return rc;
    if (!st) return EXABM4D_OK;
    char msg[160];
    std::snprintf(msg, sizeof msg, "%s: malformed label stream (status 0x%x:%s%s)", who, st,
                  st & LB_ST_MALFORMED ? " a stream, header or table entry outside its bounds" : "",
                  st & LB_ST_CLAMPED ? " a palette index >= k" : "");
    return fail(ctx, EXABM4D_ERR_INVALID, msg);
}

extern "C" {

size_t exabm4d_label_encode_bound(int typesize, int nz, int ny, int nx, int cz, int cy, int cx) {
    LabelGeom g;
    if (make_label_geom(typesize, nz, ny, nx, cz, cy, cx, g)) return 0;
    return label_volume_bound(g);
}

int exabm4d_label_encode_dev(exabm4d_ctx* ctx, const void* vol, int typesize, int nz, int ny, int nx, int cz, int cy,
                             int cx, uint8_t* out, size_t out_capacity, uint64_t* offsets_dev, uint32_t* sizes_dev,
                             uint64_t* totals_host) {
    if (!ctx || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    LabelGeom g;
    if (make_label_geom(typesize, nz, ny, nx, cz, cy, cx, g)) return fail(ctx, EXABM4D_ERR_INVALID, LB_GEOM_RULE);
    if ((uintptr_t)vol & (uintptr_t)(typesize - 1))
        return fail(ctx, EXABM4D_ERR_INVALID, "label codec: vol below the natural alignment of its elements");
    if (out) {
        if (!offsets_dev) return fail(ctx, EXABM4D_ERR_INVALID, "label codec: offsets_dev is required with out");
        if (out_capacity < label_volume_bound(g))
            return fail(ctx, EXABM4D_ERR_INVALID, "label codec: out_capacity is below exabm4d_label_encode_bound()");
        if ((uintptr_t)out & 15) return fail(ctx, EXABM4D_ERR_INVALID, "label codec: out must be 16-byte aligned");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LabelAux A;
    int rc = label_aux(ctx, g.nchunks, A);
    if (rc) return rc;
    struct Work { uint32_t *units, *blockoff; } W;
    const size_t words = (size_t)g.nchunks * g.nb;
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, W, [&](Carver& c, Work& r) {
        r.units = c.take<uint32_t>(words * 4);
        r.blockoff = c.take<uint32_t>(words * 4);
    });
    if (rc) return rc;
    if (sizes_dev) A.sizes = sizes_dev;
    if (offsets_dev) A.offsets = reinterpret_cast<unsigned long long*>(offsets_dev);
    HIP_TRY(ctx, launch_label_encode(vol, g, W.units, W.blockoff, A.sizes, A.offsets, A.totals, out, ctx->stream));
    return totals_host ? fetch(ctx, totals_host, A.totals, 2 * sizeof(uint64_t)) : EXABM4D_OK;
}

int exabm4d_label_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                             int typesize, int nz, int ny, int nx, int cz, int cy, int cx, void* vol) {
    if (!ctx || !in || !offsets_dev || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((uintptr_t)in & 15) return fail(ctx, EXABM4D_ERR_INVALID, "label codec: in must be 16-byte aligned");
    LabelGeom g;
    if (make_label_geom(typesize, nz, ny, nx, cz, cy, cx, g)) return fail(ctx, EXABM4D_ERR_INVALID, LB_GEOM_RULE);
    if ((uintptr_t)vol & (uintptr_t)(typesize - 1))
        return fail(ctx, EXABM4D_ERR_INVALID, "label codec: vol below the natural alignment of its elements");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    LabelAux A;
    int rc = label_aux(ctx, g.nchunks, A);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(A.status, 0, 16, ctx->stream));
    HIP_TRY(ctx, launch_label_decode(in, in_bytes, reinterpret_cast<const unsigned long long*>(offsets_dev), g, vol,
                                     A.status, ctx->stream));
    return label_status(ctx, A.status, "label codec");
}

int exabm4d_label_gather_boxes_dev(exabm4d_ctx* ctx, const uint8_t* data, size_t data_bytes, int typesize,
                                   const exabm4d_label_src* srcs_host, int nsrc, const int32_t* box_srcs_host,
                                   int per_box, const int32_t* starts_host, int nbox, int bz, int by, int bx,
                                   const int32_t* shape3_host, const int32_t* chunk3_host, void* out) {
    const char* who = "label_gather_boxes";
    const std::string name(who);
    if (!ctx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (typesize != 4 && typesize != 8) return fail(ctx, EXABM4D_ERR_INVALID, name + ": typesize must be 4 or 8");
    if (!shape3_host || !chunk3_host) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nbox < 0 || nsrc < 0 || per_box < 0 || bz < 1 || by < 1 || bx < 1)
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": bad sizes");
    long long voxels = 1;
    for (int a = 0; a < 3; a++) {
        if (shape3_host[a] < 1 || chunk3_host[a] < 1) return fail(ctx, EXABM4D_ERR_INVALID, name + ": bad sizes");
        voxels *= shape3_host[a];
    }
    if (voxels > (1ll << 40)) return fail(ctx, EXABM4D_ERR_INVALID, name + ": volume too large");
    if ((unsigned long long)bz * by >= (1ull << 31) || (unsigned long long)bz * by * bx > (1ull << 40) ||
        (unsigned long long)bz * by * bx * (unsigned long long)nbox > (1ull << 40) ||
        (unsigned long long)nbox * (unsigned long long)per_box > (1ull << 31))
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": boxes, batch or source lists too large");
    if (nbox == 0) return EXABM4D_OK;
    if (!out || !starts_host || (nsrc && (!data || !srcs_host)) || (per_box && !box_srcs_host))
        return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (((uintptr_t)data & 15) || ((uintptr_t)out & (uintptr_t)(typesize - 1)))
        return fail(ctx, EXABM4D_ERR_INVALID, name + ": data must be 16-byte aligned, out aligned to its elements");
    const int32_t box[3] = {bz, by, bx};
    for (int i = 0; i < nsrc; i++) {
        const exabm4d_label_src& s = srcs_host[i];
        const int32_t o[3] = {s.z0, s.y0, s.x0}, e[3] = {s.ez, s.ey, s.ex};
        unsigned long long nblk = 1;
        for (int a = 0; a < 3; a++) {
            if (o[a] < 0 || o[a] >= shape3_host[a] || o[a] % chunk3_host[a] ||
                e[a] != std::min(chunk3_host[a], shape3_host[a] - o[a]))
                return fail(ctx, EXABM4D_ERR_INVALID, name + ": a source is not a chunk of the array");
            nblk *= (unsigned long long)((e[a] + 7) / 8);
        }
        if ((s.offset & 7) || s.offset > data_bytes || s.bytes > data_bytes - s.offset || s.bytes >= (1ull << 32) ||
            nblk >= (1ull << 28) || s.bytes < LB_HEADER + 8ull * nblk)
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": a source stream outside the data, or shorter than its table");
    }
    for (int n = 0; n < nbox; n++) {
        long long lo[3], cnt[3];
        bool inside = true;
        for (int a = 0; a < 3; a++) {
            const long long s0 = starts_host[3 * n + a];
            inside = inside && s0 < shape3_host[a] && s0 + box[a] > 0;
            lo[a] = std::max(s0, 0ll) / chunk3_host[a];
            cnt[a] = (std::min(s0 + box[a], (long long)shape3_host[a]) - 1) / chunk3_host[a] - lo[a] + 1;
        }
        if (!inside) continue;                      // wholly outside the array: all zeros, no list entry is read
        if (cnt[0] * cnt[1] * cnt[2] > per_box)
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": a box touches more chunks than per_box");
        const int32_t* list = box_srcs_host + (size_t)n * per_box;
        size_t j = 0;
        for (long long z = 0; z < cnt[0]; z++)
            for (long long y = 0; y < cnt[1]; y++)
                for (long long x = 0; x < cnt[2]; x++, j++) {
                    if (list[j] < 0 || list[j] >= nsrc)
                        return fail(ctx, EXABM4D_ERR_INVALID, name + ": a source list entry outside [0, nsrc)");
                    const exabm4d_label_src& s = srcs_host[list[j]];
                    if (s.z0 != (lo[0] + z) * chunk3_host[0] || s.y0 != (lo[1] + y) * chunk3_host[1] ||
                        s.x0 != (lo[2] + x) * chunk3_host[2])
                        return fail(ctx, EXABM4D_ERR_INVALID, name + ": a source list is not the box's chunk range");
                }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the tables on the device (the copies out of pageable host memory are staged before they return)
    struct Tables { LabelChunkSrc* srcs; int32_t *lists, *starts; uint32_t* status; } L;
    const size_t nlist = (size_t)nbox * per_box;
    int rc = carve(ctx, ctx->region_tab, 0, L, [&](Carver& c, Tables& r) {
        r.srcs = c.take<LabelChunkSrc>((size_t)nsrc * sizeof(LabelChunkSrc));
        r.lists = c.take<int32_t>(nlist * 4);
        r.starts = c.take<int32_t>((size_t)nbox * 12);
        r.status = c.take<uint32_t>(16);
    });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (nsrc) HIP_TRY(ctx, hipMemcpyAsync(L.srcs, srcs_host, (size_t)nsrc * sizeof(LabelChunkSrc), hipMemcpyHostToDevice, s));
    if (nlist) HIP_TRY(ctx, hipMemcpyAsync(L.lists, box_srcs_host, nlist * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(L.starts, starts_host, (size_t)nbox * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(L.status, 0, 16, s));
    HIP_TRY(ctx, launch_label_gather(data, typesize, L.srcs, L.lists, per_box, L.starts, nbox, bz, by, bx, shape3_host,
                                     chunk3_host, out, L.status, s));
    return label_status(ctx, L.status, who);
}

}  // extern "C"
