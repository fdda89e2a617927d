// exabm4d_api.hip -- the C-ABI of libexabm4d.so (include/exabm4d.h): context lifecycle, options, memory and
// event helpers, tables and geometry, and the helpers the entry points share (exabm4d_api.h).  The entry points
// of each subsystem are in api_*.hip.  Host code only; kernels live in *_kernels.hip.
#include <initializer_list>
#include <new>

#include "exabm4d_api.h"

using namespace exabm4d;

static thread_local std::string g_err;

namespace exabm4d {

int fail(exabm4d_ctx* ctx, int code, const std::string& msg) {
    g_err = msg;
    if (ctx) ctx->err = msg;
    return code;
}

// ---- tables -----------------------------------------------------------------
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0, q = x * x / 4.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
void make_tables(double beta, float* dct64, float* win512, float* win1d) {
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; u++)
        for (int n = 0; n < 8; n++) {
            const double c = (u == 0) ? std::sqrt(1.0 / 8.0) : std::sqrt(2.0 / 8.0);
            dct64[u * 8 + n] = (float)(c * std::cos(pi * (2.0 * n + 1.0) * u / 16.0));
        }
    double k[8];
    for (int n = 0; n < 8; n++) {
        if (beta == 0.0) {
            k[n] = 1.0;
        } else {
            const double r = 2.0 * n / 7.0 - 1.0;
            k[n] = bessel_i0(beta * std::sqrt(1.0 - r * r)) / bessel_i0(beta);
        }
    }
    for (int z = 0; z < 8; z++)
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) win512[(z * 8 + y) * 8 + x] = (float)(k[z] * k[y] * k[x]);
    if (win1d)
        for (int n = 0; n < 8; n++) win1d[n] = (float)k[n];
}
const float* dct_table() {
    static float dct[64], win[512];
    static const bool made = (make_tables(0.0, dct, win), true);     // once, thread-safe
    (void)made;
    return dct;
}

int check_params(exabm4d_ctx* ctx, const exabm4d_params* p) {
    if (!p) return fail(ctx, EXABM4D_ERR_INVALID, "params is NULL");
    if (p->size != sizeof(exabm4d_params))
        return fail(ctx, EXABM4D_ERR_INVALID, "params.size does not match this library");
    if (p->block != 8 || p->step != 4 || p->search != 11 || p->max_group != 16)
        return fail(ctx, EXABM4D_ERR_UNSUPPORTED,
                    "only block=8, step=4, search=11, max_group=16 are implemented");
    if (!(p->lambda_ht >= 0.0f) || !(p->c_match_ht > 0.0f) || !(p->c_match_wie > 0.0f) ||
        !(p->kaiser_beta >= 0.0f))
        return fail(ctx, EXABM4D_ERR_INVALID, "params: thresholds must be positive, beta >= 0");
    return EXABM4D_OK;
}
int make_geom(exabm4d_ctx* ctx, int nz, int ny, int nx, int batch, VolGeom& g) {
    if (nz < 8 || ny < 8 || nx < 8) return fail(ctx, EXABM4D_ERR_INVALID, "every volume axis must be >= 8");
    if (batch < 1 || batch > 65535) return fail(ctx, EXABM4D_ERR_INVALID, "batch must be in [1, 65535]");
    g.nz = nz; g.ny = ny; g.nx = nx;
    g.gz = grid_count(nz); g.gy = grid_count(ny); g.gx = grid_count(nx);
    g.az = aligned_count(nz); g.ay = aligned_count(ny); g.ax = aligned_count(nx);
    g.nvox = (long long)nz * ny * nx;
    g.nref = (long long)g.gz * g.gy * g.gx;
    if (g.nref > 0x7FFFFFFFLL) return fail(ctx, EXABM4D_ERR_INVALID, "volume too large for one launch");
    if ((long long)ny * nx * 24 * 4 > 0xFFFFFFFFLL)
        return fail(ctx, EXABM4D_ERR_INVALID, "z-plane too large (24 planes must fit 32-bit byte offsets)");
    return EXABM4D_OK;
}
int ensure_window(exabm4d_ctx* ctx, double beta) {
    if (ctx->win_dev.p && ctx->win_beta == beta) return EXABM4D_OK;
    make_tables(beta, ctx->dct, ctx->win, ctx->win1d);
    if (!ctx->win_dev.p) {
        HIP_TRY(ctx, hipMalloc(&ctx->win_dev.p, sizeof ctx->win));
        ctx->win_dev.bytes = sizeof ctx->win;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->win_dev.p, ctx->win, sizeof ctx->win, hipMemcpyHostToDevice));
    ctx->win_beta = beta;
    return EXABM4D_OK;
}
bool guarded_region_ok(const exabm4d_ctx* ctx, const void* ptr, size_t bytes) {
    const char* lo = ctx->scratch.as<const char>();
    const char* hi = lo + ctx->scratch.bytes + GUARD_BYTES;      // ensure_scratch allocates + GUARD_BYTES
    const char* p = static_cast<const char*>(ptr);
    return lo && p >= lo + GUARD_BYTES && p + bytes + GUARD_BYTES <= hi;
}
int grow(exabm4d_ctx* ctx, DevBuf& buf, size_t bytes, size_t guard) {
    if (bytes <= buf.bytes) return EXABM4D_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->side) HIP_TRY(ctx, hipStreamSynchronize(ctx->side));   // (memsets of a call that failed half way)
    if (ctx->copy_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    if (buf.p) (void)hipFree(buf.p);
    buf = DevBuf();
    hipError_t e = hipMalloc(&buf.p, bytes + guard);
    if (e != hipSuccess) {
        buf.p = nullptr;
        char msg[160];
        std::snprintf(msg, sizeof msg, "device scratch allocation of %zu bytes failed: %s", bytes,
                      hipGetErrorString(e));
        return fail(ctx, EXABM4D_ERR_NOMEM, msg);
    }
    buf.bytes = bytes;
    return EXABM4D_OK;
}
// The kernels raise bits of the context's status word instead of hanging (block matching's carry: bm_kernels.hip
// ORDER).  Looked at, and cleared, wherever the host has just synchronised with the context's stream; `fired` gets
// the bits.  With both set the carry's error is returned: host_batch repeats the run, and the repeat reports bit 1.
int check_async_status(exabm4d_ctx* ctx, unsigned* fired) {
    const unsigned bits = ctx->status_host ? *ctx->status_host : 0u;
    if (fired) *fired = bits;
    if (bits == 0) return EXABM4D_OK;
    *ctx->status_host = 0;
    if (bits & 1u) {
        ctx->bm.carry = 0;       // the assumption behind the carry failed on this device: do without it from now on
        return fail(ctx, EXABM4D_ERR_HIP,
                    "block matching: a tile waited for the tile below it longer than the poll limit (carry between "
                    "tiles, DESIGN.md 5.1c); the match tables of the calls since the last synchronisation are void. "
                    "The carry is now off for this context (option bm_carry = 0): repeat the call.");
    }
    if (bits & 2u)
        return fail(ctx, EXABM4D_ERR_INVALID,
                    "fp32 input outside the working range of the specification: a volume holds |v| >= 2^56, an "
                    "infinity or a NaN (the squares of its transform coefficients leave fp32, DESIGN.md 3.8); the "
                    "results of the calls since the last synchronisation are void");
    return fail(ctx, EXABM4D_ERR_HIP, "a kernel reported an unknown status bit");
}
// + GUARD_BYTES: block matching reads up to 124 bytes past the last row of the library's own volumes (bm_tile_kernel,
// `guarded`); the region in front of each of them is another scratch region (checked per launch: guarded_region_ok)
int ensure_scratch(exabm4d_ctx* ctx, size_t bytes) { return grow(ctx, ctx->scratch, bytes, GUARD_BYTES); }
int fetch(exabm4d_ctx* ctx, void* host, const void* dev, size_t bytes) {
    HIP_TRY(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return EXABM4D_OK;
}

}  // namespace exabm4d

extern "C" {

int exabm4d_version(void) { return EXABM4D_VERSION; }

const char* exabm4d_last_error(const exabm4d_ctx* ctx) {
    if (ctx && !ctx->err.empty()) return ctx->err.c_str();
    return g_err.c_str();
}

int exabm4d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int exabm4d_create(int device, exabm4d_ctx** out) {
    if (!out) return fail(nullptr, EXABM4D_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, EXABM4D_ERR_NODEVICE, "no HIP device visible (libexabm4d needs a gfx950 GPU)");
    if (device < 0 || device >= n) return fail(nullptr, EXABM4D_ERR_INVALID, "device index out of range");
    HIP_TRY(nullptr, hipSetDevice(device));
    exabm4d_ctx* ctx = new (std::nothrow) exabm4d_ctx();
    if (!ctx) return fail(nullptr, EXABM4D_ERR_NOMEM, "out of host memory");
    ctx->device = device;
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail_hip(nullptr, e, "hipStreamCreate");
    }
    ctx->own_stream = true;
    e = hipHostMalloc((void**)&ctx->status_host, sizeof(unsigned), hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&ctx->status_dev, ctx->status_host, 0);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(ctx->stream);
        if (ctx->status_host) (void)hipHostFree(ctx->status_host);
        delete ctx;
        return fail_hip(nullptr, e, "status word (hipHostMalloc)");
    }
    *ctx->status_host = 0;
    e = hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ctx->side_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)exabm4d_destroy(ctx);
        return fail_hip(nullptr, e, "second stream (hipStreamCreate / hipEventCreate)");
    }
    *out = ctx;
    return EXABM4D_OK;
}

int exabm4d_destroy(exabm4d_ctx* ctx) {
    if (!ctx) return EXABM4D_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side);
        (void)hipStreamDestroy(ctx->side);
    }
    for (int i = 0; i < 2; i++)
        if (ctx->side_ev[i]) (void)hipEventDestroy(ctx->side_ev[i]);
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    for (int i = 0; i < 3; i++)
        if (ctx->copy_ev[i]) (void)hipEventDestroy(ctx->copy_ev[i]);
    for (DevBuf* b : {&ctx->scratch, &ctx->red, &ctx->rcp_dev, &ctx->codec_aux, &ctx->win_dev, &ctx->tf_lut,
                      &ctx->region_tab})
        if (b->p) (void)hipFree(b->p);
    if (ctx->region_host) (void)hipHostFree(ctx->region_host);
    if (ctx->region_ev) (void)hipEventDestroy(ctx->region_ev);
    if (ctx->status_host) (void)hipHostFree(ctx->status_host);
    for (int i = 0; i < 2 * EXABM4D_PHASE_COUNT; i++)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return EXABM4D_OK;
}

int exabm4d_set_stream(exabm4d_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, EXABM4D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;   // NULL = the HIP null stream (PyTorch's default)
    ctx->own_stream = false;
    return EXABM4D_OK;
}

int exabm4d_reset_stream(exabm4d_ctx* ctx) {
    if (!ctx) return fail(nullptr, EXABM4D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) return check_async_status(ctx);
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
    return check_async_status(ctx);
}

int exabm4d_sync(exabm4d_ctx* ctx) {
    if (!ctx) return fail(nullptr, EXABM4D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_async_status(ctx);
}

int exabm4d_default_params(exabm4d_params* p) {
    if (!p) return fail(nullptr, EXABM4D_ERR_INVALID, "params is NULL");
    p->size = sizeof(exabm4d_params);
    p->block = 8;
    p->step = 4;
    p->search = 11;
    p->max_group = 16;
    p->lambda_ht = 2.7f;
    p->c_match_ht = 3.0f;
    p->c_match_wie = 0.6f;
    p->kaiser_beta = 2.0f;
    return EXABM4D_OK;
}

int exabm4d_set_option(exabm4d_ctx* ctx, const char* name, int value) {
    if (!ctx || !name) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (std::strcmp(name, "force_generic_bm") == 0) {
        ctx->force_generic_bm = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_guarded_copy") == 0) {
        ctx->bm_guarded_copy = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "codec_version") == 0) {
        if (value != 1 && value != 2) return fail(ctx, EXABM4D_ERR_INVALID, "codec_version must be 1 or 2");
        ctx->codec_version = value;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_int") == 0) {
        ctx->bm_int = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "stage_pairvol") == 0) {      // Wiener gathers from an interleaved (noisy, basic) volume
        ctx->stage.pairvol = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_carry") == 0) {           // block matching: carry between the tiles of a column (0 off, 1 automatic, 2 forced)
        if (value < 0 || value > 2) return fail(ctx, EXABM4D_ERR_INVALID, "bm_carry must be 0, 1 or 2");
        ctx->bm.carry = value;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_layers") == 0) {          // integer block matching: cell layers per tile (0 automatic, 8 or 12 forced)
        if (value != 0 && value != 8 && value != 12) return fail(ctx, EXABM4D_ERR_INVALID, "bm_layers must be 0, 8 or 12");
        ctx->bm.layers = value;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "host_pipeline") == 0) {      // exabm4d_denoise_f32_host: large batches in overlapped sub-batches
        ctx->host_pipeline = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "zero_overlap") == 0) {       // the sums' memsets under block matching (second stream) or in line
        ctx->zero_overlap = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_carry_fault") == 0) {     // debug: every carry wait counts as run out (error-path test)
        ctx->bm.carry_fault = value ? 1 : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "bm_xcd_mode") == 0) {        // block matching's workgroup order (bm_kernels.hip)
        ctx->bm.xcd_mode = value < 0 ? 0 : (value > 16 ? 16 : value);   // >= 2: strips of that many tile rows
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "stage_strip") == 0) {        // tile-column order of the two-waves-per-group stage kernels (0 = raster, n = strips of n tile rows)
        ctx->stage.strip = value > 0 ? value : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "stage_chunks") == 0) {       // diagnostic: z chunks of the stage kernels
        ctx->stage.chunks = value > 0 ? value : 0;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "chunk_budget_mb") == 0) {
        if (value < 1) return fail(ctx, EXABM4D_ERR_INVALID, "chunk_budget_mb must be >= 1");
        ctx->chunk_budget_mb = value;
        return EXABM4D_OK;
    }
    if (std::strcmp(name, "profile") == 0) {
        if (value && !ctx->ev[0])
            for (int i = 0; i < 2 * EXABM4D_PHASE_COUNT; i++) HIP_TRY(ctx, hipEventCreate(&ctx->ev[i]));
        ctx->profile = value ? 1 : 0;
        return EXABM4D_OK;
    }
    return fail(ctx, EXABM4D_ERR_INVALID, std::string("unknown option: ") + name);
}

// ---- memory helpers --------------------------------------------------------------------------------
int exabm4d_malloc(exabm4d_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    *dptr = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(ctx, EXABM4D_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return EXABM4D_OK;
}
int exabm4d_free(exabm4d_ctx* ctx, void* dptr) {
    if (!ctx) return fail(nullptr, EXABM4D_ERR_INVALID, "ctx is NULL");
    if (dptr) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(dptr));
    }
    return EXABM4D_OK;
}
int exabm4d_memcpy_h2d(exabm4d_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || (!dst && bytes) || (!src && bytes)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_memcpy_d2h(exabm4d_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || (!dst && bytes) || (!src && bytes)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (int rc = fetch(ctx, dst, src, bytes)) return rc;
    return check_async_status(ctx);
}
int exabm4d_memset(exabm4d_ctx* ctx, void* dst, int value, size_t bytes) {
    if (!ctx || (!dst && bytes)) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_event_create(exabm4d_ctx* ctx, void** ev) {
    if (!ctx || !ev) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    hipEvent_t e;
    HIP_TRY(ctx, hipEventCreate(&e));
    *ev = (void*)e;
    return EXABM4D_OK;
}
int exabm4d_event_destroy(exabm4d_ctx* ctx, void* ev) {
    if (!ctx) return fail(nullptr, EXABM4D_ERR_INVALID, "ctx is NULL");
    if (ev) HIP_TRY(ctx, hipEventDestroy((hipEvent_t)ev));
    return EXABM4D_OK;
}
int exabm4d_event_record(exabm4d_ctx* ctx, void* ev) {
    if (!ctx || !ev) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipEventRecord((hipEvent_t)ev, ctx->stream));
    return EXABM4D_OK;
}
int exabm4d_event_elapsed_ms(exabm4d_ctx* ctx, void* a, void* b, float* ms) {
    if (!ctx || !a || !b || !ms) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipEventSynchronize((hipEvent_t)b));
    HIP_TRY(ctx, hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return EXABM4D_OK;
}

// ---- geometry + tables --------------------------------------------------------------------------------
int exabm4d_grid_count(int n) { return grid_count(n); }
int exabm4d_grid_positions(int n, int32_t* pos) {
    if (!pos) return fail(nullptr, EXABM4D_ERR_INVALID, "pos is NULL");
    const int c = grid_count(n), a = aligned_count(n);
    for (int i = 0; i < c; i++) pos[i] = grid_pos(i, a, n);
    return EXABM4D_OK;
}
int exabm4d_tables(const exabm4d_params* p, float* dct64, float* win512) {
    int rc = check_params(nullptr, p);
    if (rc) return rc;
    if (!dct64 || !win512) return fail(nullptr, EXABM4D_ERR_INVALID, "NULL argument");
    make_tables((double)p->kaiser_beta, dct64, win512);
    return EXABM4D_OK;
}
int exabm4d_blockmatch_plan(const exabm4d_ctx* ctx, int nz, int ny, int nx, int batch, int32_t plan[6],
                            uint64_t* carry_bytes) {
    if (!plan || !carry_bytes) return EXABM4D_ERR_INVALID;
    VolGeom g;
    const int rc = make_geom(nullptr, nz, ny, nx, batch, g);
    if (rc) return rc;
    const BmPlan p = bm_plan(g, batch, ctx ? ctx->bm : BmOpts());
    // plan[0] counts tiles of EIGHT cell layers, the fp32 kernel's launch of this plan, as it always has; where the
    // integer kernel takes 12 layers per tile (bm_layers) its launch has fewer slabs (BmPlan::tz)
    plan[0] = p.tz_f32; plan[1] = p.ty; plan[2] = p.tx; plan[3] = p.xq; plan[4] = p.carry; plan[5] = p.flat;
    *carry_bytes = (uint64_t)p.carry_bytes;
    return EXABM4D_OK;
}

// Page-lock caller memory that host entry points will copy from / to many times (the broker: every worker's
// shared-memory segment, for the life of the connection): the copies then are DMA transfers instead of staged
// ones.  hipHostRegisterDefault; the mapping is per process, the registration per (pointer, size).
int exabm4d_host_register(exabm4d_ctx* ctx, void* ptr, size_t bytes) {
    if (!ctx || !ptr || !bytes) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument or empty range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return EXABM4D_OK;
}
int exabm4d_host_unregister(exabm4d_ctx* ctx, void* ptr) {
    if (!ctx || !ptr) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipHostUnregister(ptr));
    return EXABM4D_OK;
}

int exabm4d_profile_read(exabm4d_ctx* ctx, float* ms, int max_phases) {
    if (!ctx || !ms) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    if (!ctx->ev[0]) return fail(ctx, EXABM4D_ERR_INVALID, "profiling was never enabled");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int n = max_phases < EXABM4D_PHASE_COUNT ? max_phases : EXABM4D_PHASE_COUNT;
    for (int i = 0; i < n; i++) {
        ms[i] = 0.0f;
        if (ctx->ev_used[i]) HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->ev[2 * i], ctx->ev[2 * i + 1]));
    }
    return n;
}

}  // extern "C"
