// api_codec.hip -- chunk byte histograms, the DCT quantiser, the EXAC chunk codec and the two error-bounded codecs.
// Host code only; the context and the shared helpers are in exabm4d_api.h.
#include "exabm4d_api.h"

using namespace exabm4d;

// ---- chunk entropy coder: scratch, tables and the checks both encoders and decoders share -------
// aux layout: sizes u32[nchunks] | offsets u64[nchunks + 1] | totals u64[2] | status u32[4]
struct CodecAux { uint32_t* sizes; unsigned long long *offsets, *totals; uint32_t* status; };
static int codec_aux(exabm4d_ctx* ctx, int nchunks, CodecAux& A) {
    return carve(ctx, ctx->codec_aux, 0, A, [&](Carver& c, auto& r) {
        r.sizes = c.take<uint32_t>((size_t)nchunks * 4);
        r.offsets = c.take<unsigned long long>(((size_t)nchunks + 1) * 8);
        r.totals = c.take<unsigned long long>(2 * 8);
        r.status = c.take<uint32_t>(4 * 4);
    });
}
// the rANS coders' reciprocal table, uploaded once per context
static int codec_rcp(exabm4d_ctx* ctx) {
    if (!ctx->rcp_dev.p) {
        static uint32_t tab[4097 * 2];
        codec_fill_rcp_table(tab);
        HIP_TRY(ctx, hipMalloc(&ctx->rcp_dev.p, sizeof tab));
        ctx->rcp_dev.bytes = sizeof tab;
        HIP_TRY(ctx, hipMemcpy(ctx->rcp_dev.p, tab, sizeof tab, hipMemcpyHostToDevice));
    }
    return EXABM4D_OK;
}
// The encoders' output container: offsets_dev with it, room for the volume bound, 16-byte aligned.  `who` and
// `bound_fn` name the encoder and its bound in the messages.
static int check_container(exabm4d_ctx* ctx, const std::string& who, const char* bound_fn, size_t bound,
                           const uint8_t* out, size_t out_capacity, const uint64_t* offsets_dev) {
    if (!out) return EXABM4D_OK;
    if (!offsets_dev) return fail(ctx, EXABM4D_ERR_INVALID, who + ": offsets_dev is required with out");
    if (out_capacity < bound)
        return fail(ctx, EXABM4D_ERR_INVALID, who + ": out_capacity is below " + bound_fn + "()");
    if ((uintptr_t)out & 15) return fail(ctx, EXABM4D_ERR_INVALID, who + ": out must be 16-byte aligned");
    return EXABM4D_OK;
}
// The decoders' status word, fetched after the last kernel: nonzero is a malformed chunk stream.
static int check_stream_status(exabm4d_ctx* ctx, const uint32_t* status, const char* who) {
    uint32_t st = 0;
    if (int rc = fetch(ctx, &st, status, sizeof st)) return rc;
    if (!st) return EXABM4D_OK;
    char msg[96];
    std::snprintf(msg, sizeof msg, "%s: malformed chunk stream (status 0x%x)", who, st);
    return fail(ctx, EXABM4D_ERR_INVALID, msg);
}

// ---- the two error-bounded lossy chunk codecs: step ladder, geometry, volume bounds -----
// The step ladder Q[j] = (float) 2^((j - 4) / 4): the kernels take it as a table, none of them computes it.
struct BqLadder {
    float q[BQ_STEPS];
    BqLadder() {
        for (int j = 0; j < BQ_STEPS; j++) q[j] = (float)std::pow(2.0, (j - 4) / 4.0);
    }
};
static const BqLadder& bq_ladder() {
    static const BqLadder t;
    return t;
}

static int bq_geom(exabm4d_ctx* ctx, int nz, int ny, int nx, int cz, int cy, int cx, BoundedGeom& g, CodecGeom& lossy,
                   CodecGeom& lossless) {
    if (make_bounded_geom(nz, ny, nx, cz, cy, cx, g) ||
        make_codec_geom(4, g.nchunks * g.nb, 8, 64, g.nb, 8, 64, lossy, 2) ||
        make_codec_geom(2, nz, ny, nx, cz, cy, cx, lossless, 2))
        return fail(ctx, EXABM4D_ERR_INVALID,
                    "bounded codec: sizes >= 1, chunk axes multiples of 8 in [8, 65528], chunk <= 2^28 voxels");
    return EXABM4D_OK;
}

static size_t bq_volume_bound(const BoundedGeom& g) {
    const size_t a = codec_chunk_bound((size_t)g.nb * BVOX, 4), b = codec_chunk_bound((size_t)g.cz * g.cy * g.cx, 2);
    return (size_t)g.nchunks * (BQ_HEADER + ((std::max(a, b) + 15) & ~(size_t)15));
}

// The block-bounded codec has the bounded codec's geometry and ladder.  A mode-1 stream of its is
// stored only when it is shorter than the mode-0 one, so the lossless bound holds every stream.
static size_t bb_volume_bound(const BoundedGeom& g) {
    const size_t b = codec_chunk_bound((size_t)g.cz * g.cy * g.cx, 2);
    return (size_t)g.nchunks * (BQ_HEADER + ((b + 15) & ~(size_t)15));
}

static int bq_upload_ladder(exabm4d_ctx* ctx, float* qtab) {
    HIP_TRY(ctx, hipMemcpyAsync(qtab, bq_ladder().q, sizeof(BqLadder), hipMemcpyHostToDevice, ctx->stream));
    return EXABM4D_OK;
}

// ---- what the entries of the two error-bounded codecs share ------------------------------------------------------
// An encode: geometry, and the scratch -- ladder, indices, the two candidate streams, the container, and last the
// codec's own regions (`own` of bq_encode_begin).
struct BqEncode {
    BoundedGeom g;
    CodecGeom gl, gu;                                    // the chunk coder's view of the indices, and of the voxels
    float* qtab;
    int32_t* idx;
    uint32_t *lsz, *usz, *sizes;
    unsigned long long *loff, *uoff, *tot, *offsets;     // tot: lossy, lossless, container {exact, container}
    uint8_t *lbuf, *ubuf, *slot;
    uint32_t* err;                                       // bounded: per-step errors, then the choices j* and Q[j*]
    int32_t* jsel;
    float* qsel;
    uint8_t* plane;                                      // block-bounded: step planes
};
// Checks behind the entry's own, scratch, ladder upload (the first thing on the stream).  `who` names the codec,
// `bound` / `bound_fn` its volume bound.
template <typename Own>
static int bq_encode_begin(exabm4d_ctx* ctx, const char* who, size_t (*bound)(const BoundedGeom&), const char* bound_fn,
                           int nz, int ny, int nx, int cz, int cy, int cx, uint8_t* out, size_t out_capacity,
                           uint64_t* offsets_dev, uint32_t* sizes_dev, BqEncode& E, Own own) {
    int rc = bq_geom(ctx, nz, ny, nx, cz, cy, cx, E.g, E.gl, E.gu);
    if (rc) return rc;
    rc = check_container(ctx, who, bound_fn, bound(E.g), out, out_capacity, offsets_dev);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = codec_rcp(ctx);
    if (rc) return rc;
    const size_t nc = (size_t)E.g.nchunks;
    const size_t slots = std::max(align256((size_t)E.gl.nchunks * E.gl.slot_bytes) + codec2_work_bytes(E.gl),
                                  align256((size_t)E.gu.nchunks * E.gu.slot_bytes) + codec2_work_bytes(E.gu));
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, E, [&](Carver& c, auto& r) {
        r.qtab = c.take<float>(sizeof(BqLadder));
        own(c, r, nc);
        r.idx = c.take<int32_t>(nc * r.g.nb * BVOX * sizeof(int32_t));
        r.lsz = c.take<uint32_t>(nc * sizeof(uint32_t));
        r.loff = c.take<unsigned long long>((nc + 1) * 8);
        r.lbuf = out ? c.take<uint8_t>(codec_volume_bound(r.gl)) : nullptr;
        r.usz = c.take<uint32_t>(nc * sizeof(uint32_t));
        r.uoff = c.take<unsigned long long>((nc + 1) * 8);
        r.ubuf = out ? c.take<uint8_t>(codec_volume_bound(r.gu)) : nullptr;
        r.tot = c.take<unsigned long long>(6 * 8);
        r.sizes = c.take<uint32_t>(nc * sizeof(uint32_t));
        r.offsets = c.take<unsigned long long>((nc + 1) * 8);
        r.slot = c.take<uint8_t>(slots);
    });
    if (rc) return rc;
    if (sizes_dev) E.sizes = sizes_dev;
    if (offsets_dev) E.offsets = reinterpret_cast<unsigned long long*>(offsets_dev);
    return bq_upload_ladder(ctx, E.qtab);
}
// the two candidates of every chunk through the existing chunk coder: the index chunks, then the voxels
static int bq_encode_candidates(exabm4d_ctx* ctx, const uint16_t* vol, const BqEncode& E) {
    const uint32_t* rcp = ctx->rcp_dev.as<uint32_t>();
    HIP_TRY(ctx, launch_rans_encode(E.idx, E.gl, rcp, E.slot, E.lsz, E.loff, E.tot, E.lbuf, ctx->stream));
    HIP_TRY(ctx, launch_rans_encode(vol, E.gu, rcp, E.slot, E.usz, E.uoff, E.tot + 2, E.ubuf, ctx->stream));
    return EXABM4D_OK;
}
static int bq_encode_totals(exabm4d_ctx* ctx, const BqEncode& E, uint64_t* totals_host) {
    return totals_host ? fetch(ctx, totals_host, E.tot + 4, 2 * sizeof(uint64_t)) : EXABM4D_OK;
}

// A decode: geometry, and the scratch -- ladder, chunk modes, the two decode lists, indices of the mode-1 chunks; qv
// (the chunks' steps) is the bounded decoder's own.
struct BqDecode {
    BoundedGeom g;
    CodecGeom gl, gu;
    const unsigned long long* offsets;
    float* qtab;
    uint32_t *mode, *lchunk, *lstat, *status;     // lstat: list counts [2], status
    unsigned long long* lrange;
    int32_t* idx;
    float* qv;
};
// Checks, scratch, ladder upload and the zeroed list counts and status: what precedes the format's parse kernel.
template <typename Own>
static int bq_decode_begin(exabm4d_ctx* ctx, const char* who, const uint8_t* in, const uint64_t* offsets_dev, int nz,
                           int ny, int nx, int cz, int cy, int cx, const uint16_t* vol, BqDecode& D, Own own) {
    if (!ctx || !in || !offsets_dev || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((uintptr_t)in & 15) return fail(ctx, EXABM4D_ERR_INVALID, std::string(who) + ": in must be 16-byte aligned");
    int rc = bq_geom(ctx, nz, ny, nx, cz, cy, cx, D.g, D.gl, D.gu);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nc = (size_t)D.g.nchunks;
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, D, [&](Carver& c, auto& r) {
        r.qtab = c.take<float>(sizeof(BqLadder));
        r.mode = c.take<uint32_t>(nc * sizeof(uint32_t));
        own(c, r, nc);
        r.lchunk = c.take<uint32_t>(2 * nc * sizeof(uint32_t));
        r.lrange = c.take<unsigned long long>(4 * nc * 8);
        r.lstat = c.take<uint32_t>(4 * sizeof(uint32_t));
        r.idx = c.take<int32_t>(nc * r.g.nb * BVOX * sizeof(int32_t));
    });
    if (rc) return rc;
    D.offsets = reinterpret_cast<const unsigned long long*>(offsets_dev);
    D.status = D.lstat + 2;
    rc = bq_upload_ladder(ctx, D.qtab);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(D.lstat, 0, 4 * sizeof(uint32_t), ctx->stream));
    return EXABM4D_OK;
}
// the lists the parse kernel made: mode-0 chunks straight into the volume, mode-1 chunks' indices into the chunk-major
// scratch (the format's inverse follows)
static int bq_decode_lists(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const BqDecode& D, uint16_t* vol) {
    const unsigned nc = (unsigned)D.g.nchunks;
    HIP_TRY(ctx, launch_rans2_decode_list(in, in_bytes, DecodeList{D.lchunk, D.lrange, D.lstat}, nc, D.gu, vol,
                                          D.status, ctx->stream));
    const DecodeList mode1{D.lchunk + nc, D.lrange + 2 * (size_t)nc, D.lstat + 1};
    HIP_TRY(ctx, launch_rans2_decode_list(in, in_bytes, mode1, nc, D.gl, D.idx, D.status, ctx->stream));
    return EXABM4D_OK;
}

// what the block-bounded entries with a bound table check of their bounds, and their select pass
static int bb_check_bounds(exabm4d_ctx* ctx, const uint16_t* bound_table, int max_error, int fg_max_error) {
    if ((uintptr_t)bound_table & 1)
        return fail(ctx, EXABM4D_ERR_INVALID, "block-bounded codec: bound_table must be 2-byte aligned");
    if (fg_max_error < 0 || fg_max_error > max_error || max_error > 65535)
        return fail(ctx, EXABM4D_ERR_INVALID, "block-bounded codec: 0 <= fg_max_error <= max_error <= 65535");
    return EXABM4D_OK;
}
static int bb_select(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, const uint16_t* bound_table,
                     const BoundedGeom& g, const float* qtab, int max_error, int fg_max_error, uint8_t* plane,
                     int32_t* idx) {
    // the memset is for the planes' padding
    HIP_TRY(ctx, hipMemsetAsync(plane, 0, (size_t)g.nchunks * bb_plane_bytes(g), ctx->stream));
    HIP_TRY(ctx, launch_bb_select(vol, mask, bound_table, g, dct_table(), qtab, (uint32_t)max_error,
                                  (uint32_t)fg_max_error, plane, idx, ctx->stream));
    return EXABM4D_OK;
}

extern "C" {

// ---- encode front end (row f-1) ---------------------------------------------------------------------
int exabm4d_chunk_byte_histograms_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx,
                                      int cz, int cy, int cx, uint32_t* hist) {
    if (!ctx || !vol || !hist) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nz < 1 || ny < 1 || nx < 1 || cz < 1 || cy < 1 || cx < 1)
        return fail(ctx, EXABM4D_ERR_INVALID, "bad sizes");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_chunk_hist(vol, nz, ny, nx, cz, cy, cx, hist, ctx->stream));
    return EXABM4D_OK;
}

// ---- transform quantiser (row f-1) ------------------------------------------------------
int exabm4d_dctq_forward_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, float q,
                             int32_t* idx) {
    if (!ctx || !vol || !idx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nz < 1 || ny < 1 || nx < 1 || !(q > 0.0f)) return fail(ctx, EXABM4D_ERR_INVALID, "bad sizes / step");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_dctq_forward(vol, nz, ny, nx, dct_table(), q, idx, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_dctq_inverse_dev(exabm4d_ctx* ctx, const int32_t* idx, int nz, int ny, int nx, float q,
                             uint16_t* vol) {
    if (!ctx || !vol || !idx) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (nz < 1 || ny < 1 || nx < 1 || !(q > 0.0f)) return fail(ctx, EXABM4D_ERR_INVALID, "bad sizes / step");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_dctq_inverse(idx, nz, ny, nx, dct_table(), q, vol, ctx->stream));
    return EXABM4D_OK;
}

// ---- chunk entropy coder (row f-1) --------------------------------------------------------
size_t exabm4d_codec_chunk_bound(size_t n_elems, int typesize) {
    if (typesize != 2 && typesize != 4) return 0;
    return codec_chunk_bound(n_elems, typesize);
}
size_t exabm4d_codec_volume_bound(int typesize, int nz, int ny, int nx, int cz, int cy, int cx) {
    CodecGeom g;
    if (make_codec_geom(typesize, nz, ny, nx, cz, cy, cx, g)) return 0;
    return codec_volume_bound(g);
}

int exabm4d_codec_encode_dev(exabm4d_ctx* ctx, const void* vol, int typesize, int version, int nz, int ny, int nx,
                             int cz, int cy, int cx, uint8_t* out, size_t out_capacity,
                             uint64_t* offsets_dev, uint32_t* sizes_dev, uint64_t* totals_host) {
    if (!ctx || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (version < 0 || version > 2) return fail(ctx, EXABM4D_ERR_INVALID, "codec: version must be 0 (context default), 1 or 2");
    CodecGeom g;
    if (make_codec_geom(typesize, nz, ny, nx, cz, cy, cx, g, version ? version : ctx->codec_version))
        return fail(ctx, EXABM4D_ERR_INVALID, "codec: typesize must be 2 or 4, sizes >= 1, chunk <= 2^28 elements");
    int rc = check_container(ctx, "codec", "exabm4d_codec_volume_bound", codec_volume_bound(g), out, out_capacity,
                             offsets_dev);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = codec_rcp(ctx);
    if (rc) return rc;
    CodecAux A;
    rc = codec_aux(ctx, g.nchunks, A);
    if (rc) return rc;
    rc = ensure_scratch(ctx, align256((size_t)g.nchunks * g.slot_bytes) + (g.version == 2 ? codec2_work_bytes(g) : 0));
    if (rc) return rc;
    if (sizes_dev) A.sizes = sizes_dev;
    if (offsets_dev) A.offsets = reinterpret_cast<unsigned long long*>(offsets_dev);
    HIP_TRY(ctx, launch_rans_encode(vol, g, ctx->rcp_dev.as<uint32_t>(), ctx->scratch.as<uint8_t>(), A.sizes,
                                    A.offsets, A.totals, out, ctx->stream));
    return totals_host ? fetch(ctx, totals_host, A.totals, 2 * sizeof(uint64_t)) : EXABM4D_OK;
}
int exabm4d_codec_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                             int typesize, int nz, int ny, int nx, int cz, int cy, int cx, void* vol) {
    if (!ctx || !in || !offsets_dev || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if ((uintptr_t)in & 15) return fail(ctx, EXABM4D_ERR_INVALID, "codec: in must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the format version is the third byte of every chunk stream: look at the first one
    uint64_t first[2] = {0, 0};
    int rc = fetch(ctx, first, offsets_dev, sizeof first);
    if (rc) return rc;
    if (first[0] > first[1] || first[1] > in_bytes || first[1] - first[0] < 4)
        return fail(ctx, EXABM4D_ERR_INVALID, "codec: malformed chunk stream (offsets outside the buffer)");
    uint8_t magic[4] = {0, 0, 0, 0};
    rc = fetch(ctx, magic, in + first[0], 4);
    if (rc) return rc;
    if (magic[0] != 'E' || magic[1] != 'X' || (magic[2] != 1 && magic[2] != 2))
        return fail(ctx, EXABM4D_ERR_INVALID, "codec: malformed chunk stream (not an EXAC v1 / v2 stream)");
    CodecGeom g;
    if (make_codec_geom(typesize, nz, ny, nx, cz, cy, cx, g, magic[2]))
        return fail(ctx, EXABM4D_ERR_INVALID, "codec: typesize must be 2 or 4, sizes >= 1, chunk <= 2^28 elements");
    CodecAux A;
    rc = codec_aux(ctx, g.nchunks, A);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(A.status, 0, 16, ctx->stream));
    HIP_TRY(ctx, launch_rans_decode(in, in_bytes, reinterpret_cast<const unsigned long long*>(offsets_dev), g,
                                    vol, A.status, ctx->stream));
    return check_stream_status(ctx, A.status, "codec");
}

// ---- error-bounded lossy chunk codec -----------------------------------------------------------
size_t exabm4d_bounded_volume_bound(int nz, int ny, int nx, int cz, int cy, int cx) {
    BoundedGeom g;
    if (make_bounded_geom(nz, ny, nx, cz, cy, cx, g)) return 0;
    return bq_volume_bound(g);
}

int exabm4d_dctq_ladder_errors_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int cz, int cy,
                                   int cx, uint32_t* err) {
    if (!ctx || !vol || !err) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    BoundedGeom g;
    CodecGeom gl, gu;
    int rc = bq_geom(ctx, nz, ny, nx, cz, cy, cx, g, gl, gu);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ensure_scratch(ctx, align256(sizeof(BqLadder)));
    if (rc) return rc;
    float* qtab = ctx->scratch.as<float>();
    rc = bq_upload_ladder(ctx, qtab);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(err, 0, (size_t)g.nchunks * BQ_STEPS * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, launch_bq_ladder(vol, g, dct_table(), qtab, err, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_bounded_encode_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int cz, int cy, int cx,
                               int max_error, uint8_t* out, size_t out_capacity, uint64_t* offsets_dev,
                               uint32_t* sizes_dev, uint64_t* totals_host) {
    if (!ctx || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (max_error < 0 || max_error > 65535) return fail(ctx, EXABM4D_ERR_INVALID, "bounded codec: max_error must be in [0, 65535]");
    BqEncode E;
    int rc = bq_encode_begin(ctx, "bounded codec", bq_volume_bound, "exabm4d_bounded_volume_bound", nz, ny, nx, cz, cy,
                             cx, out, out_capacity, offsets_dev, sizes_dev, E, [](Carver& c, BqEncode& r, size_t nc) {
                                 r.err = c.take<uint32_t>(nc * BQ_STEPS * sizeof(uint32_t));
                                 r.jsel = c.take<int32_t>(nc * sizeof(int32_t));
                                 r.qsel = c.take<float>(nc * sizeof(float));
                             });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(E.err, 0, (size_t)E.g.nchunks * BQ_STEPS * sizeof(uint32_t), s));
    HIP_TRY(ctx, launch_bq_ladder(vol, E.g, dct_table(), E.qtab, E.err, s));
    HIP_TRY(ctx, launch_bq_select(E.err, E.g.nchunks, (uint32_t)max_error, E.qtab, E.jsel, E.qsel, s));
    HIP_TRY(ctx, launch_bq_forward(vol, E.g, dct_table(), E.qsel, E.idx, s));
    rc = bq_encode_candidates(ctx, vol, E);
    if (rc) return rc;
    HIP_TRY(ctx, launch_bq_assemble(E.g, E.jsel, E.qsel, E.lbuf, E.loff, E.lsz, E.ubuf, E.uoff, E.usz, E.sizes,
                                    E.offsets, E.tot + 4, out, s));
    return bq_encode_totals(ctx, E, totals_host);
}

int exabm4d_bounded_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                               int nz, int ny, int nx, int cz, int cy, int cx, uint16_t* vol) {
    BqDecode D;
    int rc = bq_decode_begin(ctx, "bounded codec", in, offsets_dev, nz, ny, nx, cz, cy, cx, vol, D,
                             [](Carver& c, BqDecode& r, size_t nc) { r.qv = c.take<float>(nc * sizeof(float)); });
    if (rc) return rc;
    HIP_TRY(ctx, launch_bq_parse(in, in_bytes, D.offsets, D.g, D.qtab, D.mode, D.qv, D.lchunk, D.lrange, D.lstat,
                                 D.status, ctx->stream));
    rc = bq_decode_lists(ctx, in, in_bytes, D, vol);
    if (rc) return rc;
    HIP_TRY(ctx, launch_bq_inverse(D.idx, D.g, dct_table(), D.mode, D.qv, vol, ctx->stream));
    return check_stream_status(ctx, D.status, "bounded codec");
}

// ---- error-bounded codec, a step per block and a per-voxel bound -------------------------------
size_t exabm4d_block_bounded_volume_bound(int nz, int ny, int nx, int cz, int cy, int cx) {
    BoundedGeom g;
    if (make_bounded_geom(nz, ny, nx, cz, cy, cx, g)) return 0;
    return bb_volume_bound(g);
}

int exabm4d_block_bounded_steps_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                    int nx, int cz, int cy, int cx, int max_error, int fg_max_error, uint8_t* plane) {
    return exabm4d_block_bounded_steps_tab_dev(ctx, vol, mask, nz, ny, nx, cz, cy, cx, max_error, fg_max_error, plane,
                                               nullptr);
}

int exabm4d_block_bounded_steps_tab_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                        int nx, int cz, int cy, int cx, int max_error, int fg_max_error,
                                        uint8_t* plane, const uint16_t* bound_table) {
    if (!ctx || !vol || !plane) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    int rc = bb_check_bounds(ctx, bound_table, max_error, fg_max_error);
    if (rc) return rc;
    BoundedGeom g;
    CodecGeom gl, gu;
    rc = bq_geom(ctx, nz, ny, nx, cz, cy, cx, g, gl, gu);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    struct { float* qtab; int32_t* idx; } S;
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, S, [&](Carver& c, auto& r) {
        r.qtab = c.take<float>(sizeof(BqLadder));
        r.idx = c.take<int32_t>((size_t)g.nchunks * g.nb * BVOX * sizeof(int32_t));
    });
    if (rc) return rc;
    rc = bq_upload_ladder(ctx, S.qtab);
    if (rc) return rc;
    return bb_select(ctx, vol, mask, bound_table, g, S.qtab, max_error, fg_max_error, plane, S.idx);
}

int exabm4d_block_bounded_encode_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                     int nx, int cz, int cy, int cx, int max_error, int fg_max_error, uint8_t* out,
                                     size_t out_capacity, uint64_t* offsets_dev, uint32_t* sizes_dev,
                                     uint64_t* totals_host) {
    return exabm4d_block_bounded_encode_tab_dev(ctx, vol, mask, nz, ny, nx, cz, cy, cx, max_error, fg_max_error, out,
                                                out_capacity, offsets_dev, sizes_dev, totals_host, nullptr);
}

int exabm4d_block_bounded_encode_tab_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                         int nx, int cz, int cy, int cx, int max_error, int fg_max_error,
                                         uint8_t* out, size_t out_capacity, uint64_t* offsets_dev,
                                         uint32_t* sizes_dev, uint64_t* totals_host, const uint16_t* bound_table) {
    if (!ctx || !vol) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    int rc = bb_check_bounds(ctx, bound_table, max_error, fg_max_error);
    if (rc) return rc;
    BqEncode E;
    rc = bq_encode_begin(ctx, "block-bounded codec", bb_volume_bound, "exabm4d_block_bounded_volume_bound", nz, ny, nx,
                         cz, cy, cx, out, out_capacity, offsets_dev, sizes_dev, E,
                         [](Carver& c, BqEncode& r, size_t nc) {
                             r.plane = c.take<uint8_t>(nc * bb_plane_bytes(r.g));
                         });
    if (rc) return rc;
    rc = bb_select(ctx, vol, mask, bound_table, E.g, E.qtab, max_error, fg_max_error, E.plane, E.idx);
    if (rc) return rc;
    rc = bq_encode_candidates(ctx, vol, E);
    if (rc) return rc;
    HIP_TRY(ctx, launch_bb_assemble(E.g, E.plane, E.lbuf, E.loff, E.lsz, E.ubuf, E.uoff, E.usz, E.sizes, E.offsets,
                                    E.tot + 4, out, ctx->stream));
    return bq_encode_totals(ctx, E, totals_host);
}

int exabm4d_block_bounded_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                     const uint64_t* offsets_dev, int nz, int ny, int nx, int cz, int cy, int cx,
                                     uint16_t* vol) {
    BqDecode D;
    int rc = bq_decode_begin(ctx, "block-bounded codec", in, offsets_dev, nz, ny, nx, cz, cy, cx, vol, D,
                             [](Carver&, BqDecode&, size_t) {});
    if (rc) return rc;
    HIP_TRY(ctx, launch_bb_parse(in, in_bytes, D.offsets, D.g, D.mode, D.lchunk, D.lrange, D.lstat, D.status,
                                 ctx->stream));
    rc = bq_decode_lists(ctx, in, in_bytes, D, vol);
    if (rc) return rc;
    HIP_TRY(ctx, launch_bb_inverse(D.idx, in, D.offsets, D.g, dct_table(), D.qtab, D.mode, vol, D.status, ctx->stream));
    return check_stream_status(ctx, D.status, "block-bounded codec");
}

}  // extern "C"
