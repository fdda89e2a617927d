// exabm4d_api.h -- private to the host layer of libexabm4d.so (exabm4d_api.hip, api_*.hip, comm_rccl.hip): the
// context and the helpers its entry points share.  The kernels' translation units do not include it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/exabm4d.h"
#include "exabm4d_kernels.h"

namespace exabm4d {

// A device buffer the context owns: grown by grow(), or allocated once (window, reciprocal and transform tables).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The error of the last failing call goes to the context (if any) and to the calling thread.
int fail(exabm4d_ctx* ctx, int code, const std::string& msg);
inline int fail_hip(exabm4d_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, EXABM4D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, expr)                                         \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return fail_hip((ctx), _e, #expr);   \
    } while (0)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Block matching's `guarded` variant streams whole plane rows by LDS-DMA and reads up to 124 bytes
// in front of the first and past the last row of the volume (bm_tile_kernel): such a volume must
// lie inside the scratch allocation with 256 mapped bytes on either side.
constexpr size_t GUARD_BYTES = 256;

// Carves one allocation into 256-byte aligned regions, in the order they are taken.  A pass with base == nullptr
// only adds up the bytes (`at`); carve() runs a layout that way to size the buffer, then on the allocation.
struct Carver {
    char* base = nullptr;
    size_t at = 0;
    template <typename T = char>
    T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += align256(bytes);
        return p;
    }
};

// ---- shared helpers (exabm4d_api.hip) ----
void make_tables(double beta, float* dct64, float* win512, float* win1d = nullptr);
const float* dct_table();      // the 8-point DCT-II matrix of make_tables, which does not depend on the window's beta
int check_params(exabm4d_ctx* ctx, const exabm4d_params* p);
int make_geom(exabm4d_ctx* ctx, int nz, int ny, int nx, int batch, VolGeom& g);
int ensure_window(exabm4d_ctx* ctx, double beta);
bool guarded_region_ok(const exabm4d_ctx* ctx, const void* ptr, size_t bytes);
// Grows `buf` to at least `bytes` (+ `guard` mapped bytes behind them), after every stream of the context is done
// with it; the contents are not kept.
int grow(exabm4d_ctx* ctx, DevBuf& buf, size_t bytes, size_t guard = 0);
int ensure_scratch(exabm4d_ctx* ctx, size_t bytes);     // the context's scratch, + GUARD_BYTES
int check_async_status(exabm4d_ctx* ctx, unsigned* fired = nullptr);
int fetch(exabm4d_ctx* ctx, void* host, const void* dev, size_t bytes);     // device -> host, then synchronise

// Grows `buf` (+ `guard`) to what `layout(Carver&, Layout&)` takes, then lets it set `out` to its regions in `buf`.
template <typename Layout, typename F>
int carve(exabm4d_ctx* ctx, DevBuf& buf, size_t guard, Layout& out, F&& layout) {
    Carver count;
    layout(count, out);
    if (int rc = grow(ctx, buf, count.at, guard)) return rc;
    Carver c{buf.as<char>()};
    layout(c, out);
    return EXABM4D_OK;
}

// batches of patches (the mask, coherence-gate and sampler entries): sizes the kernels' 32-bit voxel indices hold
inline int check_patches(exabm4d_ctx* ctx, int batch, int nz, int ny, int nx) {
    if (batch < 1 || nz < 1 || ny < 1 || nx < 1) return fail(ctx, EXABM4D_ERR_INVALID, "bad batch / sizes");
    if ((long long)nz * ny * nx >= (1ll << 32) || (long long)nz * ny * nx * batch > (1ll << 40))
        return fail(ctx, EXABM4D_ERR_INVALID, "patch or batch too large");
    return EXABM4D_OK;
}
inline bool bad_label_dtype(int d) { return d < EXABM4D_LBL_U8 || d > EXABM4D_LBL_I64; }

// A box inside a window: the geometry every such entry shares, checked before anything is
// launched.
inline int box_geometry(exabm4d_ctx* ctx, const char* who, const int32_t* vol, const int32_t* w0, const int32_t* wd,
                        const int32_t* b0, const int32_t* bd, BoxGeom& g) {
    const std::string name(who);
    if (!vol || !w0 || !wd || !b0 || !bd) return fail(ctx, EXABM4D_ERR_INVALID, name + ": NULL argument");
    long long voxels = 1;
    for (int a = 0; a < 3; a++) {
        g.n[a] = vol[a];
        g.w0[a] = w0[a];
        g.wd[a] = wd[a];
        g.b0[a] = b0[a];
        g.bd[a] = bd[a];
        if (vol[a] < 1 || wd[a] < 1 || bd[a] < 1) return fail(ctx, EXABM4D_ERR_INVALID, name + ": every extent must be >= 1");
        if (vol[a] > (1 << 20)) return fail(ctx, EXABM4D_ERR_INVALID, name + ": volume too large");
        voxels *= vol[a];
        // a window may run past the volume's upper faces (a reader's padding): nothing there is ever read
        if (w0[a] < 0 || w0[a] >= vol[a] || wd[a] > (1 << 21))
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": the window does not begin inside the volume");
        if (b0[a] < w0[a] || (long long)b0[a] + bd[a] > (long long)w0[a] + wd[a])
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": the box does not lie inside the window");
        if ((long long)b0[a] + bd[a] > vol[a])
            return fail(ctx, EXABM4D_ERR_INVALID, name + ": the box does not lie inside the volume");
    }
    if (voxels > (1ll << 40)) return fail(ctx, EXABM4D_ERR_INVALID, name + ": volume too large");
    return EXABM4D_OK;
}

}  // namespace exabm4d

struct exabm4d_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float dct[64];
    float win[512];
    float win1d[8];            // the window's 1-D factor (fp32), for den = C (*) win
    exabm4d::DevBuf win_dev;
    exabm4d::DevBuf tf_lut;    // 65536-entry forward table for uint16 input (asinh)
    double win_beta = -1.0;
    exabm4d::DevBuf scratch;   // + GUARD_BYTES behind its `bytes`
    exabm4d::DevBuf rcp_dev;   // chunk coder: reciprocal table, [4097][2]
    exabm4d::DevBuf codec_aux; // chunk coder: sizes / offsets / totals / status
    exabm4d::DevBuf red;       // metric entry points: histogram / partials / results
    // exabm4d_gather_boxes_dev: its tables on the device, the pinned host buffer they are copied from, and the event
    // behind the last copy out of it (the entry does not synchronise, so the next call waits for that event instead)
    exabm4d::DevBuf region_tab;
    void* region_host = nullptr;
    size_t region_host_bytes = 0;
    hipEvent_t region_ev = nullptr;
    int noise_wgs = 0;         // noise table: workgroups per launch (one per CU); 0 = noise_table_prepare() not yet run
    int measure_wgs = 0;       // measuring a box: the same; 0 = measure_prepare() not yet run
    int foreground_ready = 0;  // the foreground mask of a box: foreground_prepare() has run
    int force_generic_bm = 0;  // exabm4d_set_option("force_generic_bm")
    int bm_guarded_copy = 0;   // exabm4d_set_option("bm_guarded_copy"): staged block matching on a guarded copy
    exabm4d::StageOpts stage;  // exabm4d_set_option("stage_pairvol" / "stage_strip" / "stage_chunks")
    exabm4d::BmOpts bm;        // exabm4d_set_option("bm_xcd_mode" / "bm_carry" / "bm_carry_fault")
    // The 8-byte sums are zeroed on a second stream, under the block matching that precedes every stage
    // kernel (compute-bound, and it touches neither array): exabm4d_set_option("zero_overlap", 0) puts the
    // memsets back on the context's stream.
    int zero_overlap = 1;
    bool zero_on_side = false;  // the last zero_begin() went to the second stream
    // exabm4d_denoise_f32_host: large batches in double-buffered sub-batches ("host_pipeline" = 0: one piece)
    int host_pipeline = 1;
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_ev[3] = {nullptr, nullptr, nullptr};
    hipStream_t side = nullptr;
    hipEvent_t side_ev[2] = {nullptr, nullptr};     // [0] main -> side: the sums' last reader is done; [1] side -> main: zeroed
    unsigned* status_host = nullptr;   // one pinned, device-visible word: bit 0 = a carry wait of block matching ran out
    unsigned* status_dev = nullptr;
    int profile = 0;           // exabm4d_set_option("profile")
    int bm_int = 1;            // exabm4d_set_option("bm_int"): integer block matching on uint16 input
    int codec_version = 2;     // exabm4d_set_option("codec_version"): stream format the encoder writes
    int chunk_budget_mb = 32768;   // exabm4d_set_option("chunk_budget_mb"): scratch per batch of chunks
    hipEvent_t ev[2 * EXABM4D_PHASE_COUNT] = {};
    bool ev_used[EXABM4D_PHASE_COUNT] = {};
    std::string err;
};
