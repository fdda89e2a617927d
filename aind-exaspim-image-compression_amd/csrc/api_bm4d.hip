// api_bm4d.hip -- the BM4D entry points: staged launches, the whole pipeline on device and host data, the
// chunk-local modes.  Host code only; the context and the shared helpers are in exabm4d_api.h.
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "exabm4d_api.h"

using namespace exabm4d;

static uint32_t keymax_of(float sigma, float c_match) {
    const float tau512 = (float)((double)c_match * (double)sigma * (double)sigma * 512.0);
    uint32_t u;
    std::memcpy(&u, &tau512, 4);
    return (u & KEY_DMASK) + 0x800u;
}

namespace {
struct ChunkRun {
    int i0, count;       // chunks [i0, i0 + count) of the axis ...
    int e, lo, hi;       // ... share the core extent and the halo in front / behind
};
// chunks of `chunk` voxels tile [c0, c1) inside a buffer axis of n voxels
std::vector<ChunkRun> chunk_runs(int n, int c0, int c1, int chunk, int halo) {
    std::vector<ChunkRun> runs;
    int i = 0;
    for (int start = c0; start < c1; start += chunk, i++) {
        const int e = std::min(chunk, c1 - start);
        const int lo = std::min(halo, start), hi = std::min(halo, n - (start + e));
        if (!runs.empty() && runs.back().e == e && runs.back().lo == lo && runs.back().hi == hi)
            runs.back().count++;
        else
            runs.push_back({i, 1, e, lo, hi});
    }
    return runs;
}
}  // namespace

// Scratch layout of one pipeline run (run_pipeline below walks it in this order)
struct PipeLayout {
    uint32_t* keys; long long* num; float* basic; unsigned long long* cw; float *tmp, *pair; double* qscale;
    unsigned* maxbits; char* carry;
};
static void pipe_layout(Carver& c, PipeLayout& L, size_t n, size_t nref, int batch, int stages, size_t carry_bytes) {
    L.keys = c.take<uint32_t>(nref * MAXG * sizeof(uint32_t));
    L.num = c.take<long long>(n * sizeof(long long));                  // numerator, int64 fixed point
    L.basic = c.take<float>(stages >= 2 ? n * sizeof(float) : 0);
    L.cw = c.take<unsigned long long>(n * sizeof(unsigned long long)); // corner weights, int64 fixed point
    L.tmp = c.take<float>(n * sizeof(float));                          // x / y passes of the denominator convolution
    L.pair = c.take<float>(stages >= 2 ? 2 * n * sizeof(float) : 0);   // interleaved (noisy, basic) volume, Wiener
    L.qscale = c.take<double>((size_t)batch * 2 * sizeof(double));
    L.maxbits = c.take<unsigned>((size_t)batch * sizeof(unsigned));
    L.carry = c.take(carry_bytes);                                      // block matching's carry between tiles (BmPlan)
}

// scratch of one pipeline run under the given block-matching options (the carry's memory depends on them)
static size_t pipe_bytes(const BmOpts& bm, int nz, int ny, int nx, int batch, int stages) {
    VolGeom g;
    if (make_geom(nullptr, nz, ny, nx, batch, g) != EXABM4D_OK) return 0;
    Carver count;
    PipeLayout L;
    pipe_layout(count, L, (size_t)g.nvox * (size_t)batch, (size_t)g.nref * (size_t)batch, batch, stages,
                bm_plan(g, batch, bm).carry_bytes);
    return count.at;
}

extern "C" {

size_t exabm4d_scratch_bytes(int nz, int ny, int nx, int batch, int stages) {
    return pipe_bytes(BmOpts(), nz, ny, nx, batch, stages);     // default options; includes the carry (round 4)
}

// ---- argument checks of the BM4D entry points, in the order each entry has always reported them -----------
static int arg_checks(exabm4d_ctx* ctx, bool ptrs_ok, const exabm4d_params* p) {   // first: NULL, params
    if (!ctx || !ptrs_ok) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    return check_params(ctx, p);
}
static int geom_on_device(exabm4d_ctx* ctx, int nz, int ny, int nx, int batch, VolGeom& g) {   // last: geometry, device
    int rc = make_geom(ctx, nz, ny, nx, batch, g);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return EXABM4D_OK;
}
// the whole-pipeline entries: NULL, params, sigma, stages, then the batch geometry (pipeline_checks) or the chunk
// sizes (chunk_checks)
static int bm4d_checks(exabm4d_ctx* ctx, const void* in, const void* out, float sigma, const exabm4d_params* p,
                       int stages) {
    int rc = arg_checks(ctx, in && out, p);
    if (rc) return rc;
    if (!(sigma > 0.0f)) return fail(ctx, EXABM4D_ERR_INVALID, "sigma must be > 0");
    if (stages != 1 && stages != 2) return fail(ctx, EXABM4D_ERR_INVALID, "stages must be 1 or 2");
    return EXABM4D_OK;
}
static int pipeline_checks(exabm4d_ctx* ctx, const void* in, const void* out, int nz, int ny, int nx,
                           int batch, float sigma, const exabm4d_params* p, int stages, VolGeom& g) {
    int rc = bm4d_checks(ctx, in, out, sigma, p, stages);
    if (!rc) rc = geom_on_device(ctx, nz, ny, nx, batch, g);
    return rc ? rc : ensure_window(ctx, (double)p->kaiser_beta);
}
static int chunk_checks(exabm4d_ctx* ctx, const void* in, const void* out, int nz, int ny, int nx, int chunk,
                        int halo, float sigma, const exabm4d_params* p, int stages) {
    int rc = bm4d_checks(ctx, in, out, sigma, p, stages);
    if (!rc && (nz < 1 || ny < 1 || nx < 1 || chunk < 1 || halo < 0 || halo > 64))
        rc = fail(ctx, EXABM4D_ERR_INVALID, "chunked: sizes >= 1, chunk >= 1, 0 <= halo <= 64");
    return rc;
}
// the staged block-matching entries: NULL, params, sigma and c_match, the keys' alignment, geometry, device
static int blockmatch_checks(exabm4d_ctx* ctx, const void* vol, int nz, int ny, int nx, int batch, float sigma,
                             float c_match, const exabm4d_params* p, const uint32_t* keys, VolGeom& g) {
    int rc = arg_checks(ctx, vol && keys, p);
    if (rc) return rc;
    if (!(sigma > 0.0f) || !(c_match > 0.0f)) return fail(ctx, EXABM4D_ERR_INVALID, "sigma and c_match must be > 0");
    if (((uintptr_t)keys & 15u) != 0)       // a reference's 16 keys leave as 16-byte vectors
        return fail(ctx, EXABM4D_ERR_INVALID, "keys must be 16-byte aligned");
    return geom_on_device(ctx, nz, ny, nx, batch, g);
}
static int check_offset(exabm4d_ctx* ctx, float offset) {   // |v - offset| < 2^17: the uint16 pipelines' fixed unit
    if (std::fabs(offset) <= 65536.0f) return EXABM4D_OK;
    return fail(ctx, EXABM4D_ERR_INVALID, "offset must lie within [-65536, 65536]");
}

// The constants of the Poisson-Gaussian stabilisation: formed in double from the struct's floats,
// rounded once.
static int pg_entry(exabm4d_ctx* ctx, const exabm4d_pg_noise* n, PgDev& d) {
    if (!n) return fail(ctx, EXABM4D_ERR_INVALID, "noise is NULL");
    if (n->size != sizeof(exabm4d_pg_noise)) return fail(ctx, EXABM4D_ERR_INVALID, "noise.size does not match this library");
    if (!std::isfinite(n->gain) || !std::isfinite(n->read_noise) || !std::isfinite(n->offset))
        return fail(ctx, EXABM4D_ERR_INVALID, "noise: gain, read_noise and offset must be finite");
    if (!(n->gain > 0.0f) || !(n->read_noise >= 0.0f))
        return fail(ctx, EXABM4D_ERR_INVALID, "noise: gain must be > 0 and read_noise >= 0");
    if (n->inverse < 0 || n->inverse > 2) return fail(ctx, EXABM4D_ERR_INVALID, "noise.inverse must be 0, 1 or 2");
    int rc = check_offset(ctx, n->offset);
    if (rc) return rc;
    const double g = n->gain, r = n->read_noise;
    std::memset(&d, 0, sizeof d);
    d.inverse = n->inverse;
    d.gain = n->gain;
    d.off = n->offset;
    d.c38g2 = (float)((3.0 / 8.0) * g * g);
    d.rn2 = (float)(r * r);
    d.two_over_gain = (float)(2.0 / g);
    d.cg2 = (float)((n->inverse == 0 ? 3.0 / 8.0 : 1.0 / 8.0) * g * g);
    d.s2 = (float)((r / g) * (r / g));
    d.k1 = (float)(std::sqrt(1.5) / 4.0);
    d.k2 = (float)(11.0 / 8.0);
    d.k3 = (float)(5.0 * std::sqrt(1.5) / 8.0);
    d.d0 = (float)(2.0 * std::sqrt(3.0 / 8.0));
    return EXABM4D_OK;
}

// (float)v - offset is exact in fp32 for every uint16 v iff the offset has at most 7 fractional bits
// (17 integer bits of |v - offset| + 7 = 24) -- 0, 37, 100.5 ...; only then do two voxels of the
// fp32 counts differ by an exact integer and the integer matching kernel reproduce the float
// kernel's (and the oracle's) tables.  A percentile such as 36.73 takes the float kernel.
static bool offset_exact_in_fp32(float offset) {
    const float s = offset * 128.0f;
    return std::fabs(offset) <= 65536.0f && s == std::rint(s);
}
// Integer block matching (bm_tile16_kernel) on `vol16`, the uint16 shadow of n voxels cast with `offset`, where its
// tables equal the float kernel's: c sigma^2 512 < 2^24, even rows, counts exact in fp32, shadow
// in guarded scratch.  exabm4d_blockmatch_u16_dev casts with offset 0, which is always exact.
static bool int_match_ok(const exabm4d_ctx* ctx, float c_match, float sigma, const VolGeom& g,
                         const uint16_t* vol16, size_t n, float offset) {
    const double tau512 = (double)c_match * (double)sigma * (double)sigma * 512.0;
    return vol16 && ctx->bm_int && tau512 < 16777216.0 && (g.nx % 2) == 0 && offset_exact_in_fp32(offset) &&
           guarded_region_ok(ctx, vol16, n * sizeof(uint16_t));
}

// A uint16 pipeline run's scratch: pipe_bytes, fp32 counts, GUARD_BYTES, uint16 shadow (run_pipeline's guarded
// regions rely on this layout).
struct U16Scratch { float* f32; uint16_t* u16; };
static int u16_pipe_scratch(exabm4d_ctx* ctx, const VolGeom& g, int batch, int stages, U16Scratch& L) {
    const size_t n = (size_t)g.nvox * (size_t)batch, pipe = pipe_bytes(ctx->bm, g.nz, g.ny, g.nx, batch, stages);
    return carve(ctx, ctx->scratch, GUARD_BYTES, L, [&](Carver& c, auto& r) {
        c.take(pipe);                                  // run_pipeline's own regions
        r.f32 = c.take<float>(n * sizeof(float));
        c.take(GUARD_BYTES);
        r.u16 = c.take<uint16_t>(n * sizeof(uint16_t));
    });
}

// ---- one pipeline run: where the volume comes from, what matching may use, where the estimate goes -----------
constexpr bool CALLERS_BUFFER = false, IN_SCRATCH = true;      // PipeRun::in_scratch
struct PipeRun {
    // Input: fp32 counts on the device.  in_scratch: inside the scratch allocation, mapped memory on both sides
    // (ensure_scratch, bm_tile_kernel); a caller's own buffer is not assumed to be.  data_exp: E of the numerator's
    // unit, 17 for uint16 counts, EXABM4D_DATA_EXP_AUTO (every volume's largest |v|) for fp32.
    const float* noisy; bool in_scratch; int data_exp;
    // Matching on counts, the uint16 pipelines.  counts16: the same volume as uint16 XOR 0x8000,
    // guarded like `noisy`, cast with counts_offset; both stages then match in integer arithmetic where
    // int_match_ok admits it.  match_rounded: stage 2 matches on the basic estimate ROUNDED TO COUNTS,
    // rint(clamp(basic + counts_offset, 0, 65535)); counts16's memory (free after stage 1) takes it for the integer
    // kernel, `tmp` (dead between the stages) takes the same counts as fp32 for the float kernels.
    uint16_t* counts16; float counts_offset; bool match_rounded;
    // Output.  Under out.pg `noisy` is the stabilised volume and the last normalisation inverts.
    NormOut out;

    static PipeRun f32(const float* in, bool in_scratch, const NormOut& out) {
        return {in, in_scratch, EXABM4D_DATA_EXP_AUTO, nullptr, 0.0f, false, out};
    }
    static PipeRun counts_to_u16(const U16Scratch& v, float offset, uint16_t* out) {
        return {v.f32, IN_SCRATCH, EXABM4D_DATA_EXP_U16, v.u16, offset, true, NormOut::to_u16(out, offset)};
    }
    static PipeRun counts_in_place(const U16Scratch& v, float offset) {        // fp32 estimate over v.f32, unclipped
        return {v.f32, IN_SCRATCH, EXABM4D_DATA_EXP_U16, v.u16, offset, true, NormOut::to_f32(v.f32)};
    }
    static PipeRun stabilised_to_u16(const float* d, uint16_t* out, const PgDev* pg) {
        return f32(d, IN_SCRATCH, NormOut::to_u16_pg(out, pg));
    }
};

// ---- staged entry points ---------------------------------------------------------------------------------
int exabm4d_blockmatch_dev(exabm4d_ctx* ctx, const float* vol, int nz, int ny, int nx, int batch,
                           float sigma, float c_match, const exabm4d_params* p, uint32_t* keys) {
    VolGeom g;
    int rc = blockmatch_checks(ctx, vol, nz, ny, nx, batch, sigma, c_match, p, keys, g);
    if (rc) return rc;
    const BmPlan plan = bm_plan(g, batch, ctx->bm);
    if (ctx->bm_guarded_copy) {
        // parity hook for the pipeline's path: match on a copy inside the scratch allocation, with
        // 256 bytes of poison on either side, through the kernel's `guarded` variant
        const size_t bytes = (size_t)g.nvox * (size_t)batch * sizeof(float), padded = GUARD_BYTES + bytes + GUARD_BYTES;
        struct { char *padded, *carry; } L;
        rc = carve(ctx, ctx->scratch, GUARD_BYTES, L, [&](Carver& c, auto& r) {
            r.padded = c.take(padded);
            r.carry = c.take(plan.carry_bytes);
        });
        if (rc) return rc;
        float* copy = reinterpret_cast<float*>(L.padded + GUARD_BYTES);
        if (!guarded_region_ok(ctx, copy, bytes))
            return fail(ctx, EXABM4D_ERR_INVALID, "internal: guarded volume without mapped slack around it");
        HIP_TRY(ctx, hipMemsetAsync(L.padded, 0xFF, padded, ctx->stream));      // NaN bit patterns
        HIP_TRY(ctx, hipMemcpyAsync(copy, vol, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, launch_blockmatch(copy, g, batch, keymax_of(sigma, c_match), keys, ctx->stream,
                                       ctx->force_generic_bm, 1, nullptr, plan, L.carry, ctx->status_dev));
        return EXABM4D_OK;
    }
    rc = ensure_scratch(ctx, plan.carry_bytes);
    if (rc) return rc;
    HIP_TRY(ctx, launch_blockmatch(vol, g, batch, keymax_of(sigma, c_match), keys, ctx->stream,
                                   ctx->force_generic_bm, 0, nullptr, plan, ctx->scratch.p, ctx->status_dev));
    return EXABM4D_OK;
}

// Block matching on a uint16 volume the way the uint16 pipelines do it: fp32 counts and the biased
// uint16 copy side by side in guarded scratch, integer tile kernel where its tables are the float
// kernel's (else the float kernel), one-wave kernel for clamped last grid positions.
int exabm4d_blockmatch_u16_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int batch,
                               float sigma, float c_match, const exabm4d_params* p, uint32_t* keys) {
    VolGeom g;
    int rc = blockmatch_checks(ctx, vol, nz, ny, nx, batch, sigma, c_match, p, keys, g);
    if (rc) return rc;
    const size_t n = (size_t)g.nvox * (size_t)batch;
    const BmPlan plan = bm_plan(g, batch, ctx->bm);
    struct { float* f32; uint16_t* u16; char* carry; } L;     // each volume with GUARD_BYTES on either side
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, L, [&](Carver& c, auto& r) {
        c.take(GUARD_BYTES);
        r.f32 = c.take<float>(n * sizeof(float));
        c.take(GUARD_BYTES);
        r.u16 = c.take<uint16_t>(n * sizeof(uint16_t));
        c.take(GUARD_BYTES);
        r.carry = c.take(plan.carry_bytes);
    });
    if (rc) return rc;
    HIP_TRY(ctx, launch_counts_from_u16(vol, L.f32, n, 0.0f, ctx->stream, L.u16));
    const bool use16 = int_match_ok(ctx, c_match, sigma, g, L.u16, n, 0.0f);
    if (!guarded_region_ok(ctx, L.f32, n * sizeof(float)))
        return fail(ctx, EXABM4D_ERR_INVALID, "internal: guarded volume without mapped slack around it");
    HIP_TRY(ctx, launch_blockmatch(L.f32, g, batch, keymax_of(sigma, c_match), keys, ctx->stream,
                                   ctx->force_generic_bm, 1, use16 ? L.u16 : nullptr, plan, L.carry, ctx->status_dev));
    return EXABM4D_OK;
}

int exabm4d_match_decode(const uint32_t* keys16, int rz, int ry, int rx, int ny, int nx,
                         int64_t* idx, float* dist, int* count) {
    if (!keys16 || !idx || !dist || !count) return fail(nullptr, EXABM4D_ERR_INVALID, "NULL argument");
    int c = 0;
    for (int k = 0; k < MAXG; k++) {
        const uint32_t key = keys16[k];
        if (key == KEY_EMPTY) {
            idx[k] = -1;
            dist[k] = INFINITY;
            continue;
        }
        int dz, dy, dx;
        code_to_disp(key & KEY_CMASK, dz, dy, dx);
        idx[k] = ((int64_t)(rz + dz) * ny + (ry + dy)) * nx + (rx + dx);
        const uint32_t sb = key & KEY_DMASK;
        float s;
        std::memcpy(&s, &sb, 4);
        dist[k] = s / 512.0f;
        c++;
    }
    *count = c;
    return EXABM4D_OK;
}

int exabm4d_stage_dev(exabm4d_ctx* ctx, const float* noisy, const float* basic,
                      const uint32_t* keys, int nz, int ny, int nx, int batch, float sigma,
                      const exabm4d_params* p, int data_exp, float* num, float* den) {
    int rc = arg_checks(ctx, noisy && keys && num && den, p);
    if (rc) return rc;
    if (!(sigma > 0.0f)) return fail(ctx, EXABM4D_ERR_INVALID, "sigma must be > 0");
    if (data_exp != EXABM4D_DATA_EXP_AUTO && (data_exp < -200 || data_exp > 200))
        return fail(ctx, EXABM4D_ERR_INVALID, "data_exp must be EXABM4D_DATA_EXP_AUTO or within [-200, 200]");
    VolGeom g;
    rc = geom_on_device(ctx, nz, ny, nx, batch, g);
    if (rc) return rc;
    rc = ensure_window(ctx, (double)p->kaiser_beta);
    if (rc) return rc;
    const float thr = (float)((double)p->lambda_ht * (double)sigma);
    const float sigma2 = (float)((double)sigma * (double)sigma);
    const size_t n = (size_t)g.nvox * (size_t)batch;
    // int64 numerator, int64 corner weights (adjacent: one memset), fp32 ping-pong, [pair volume], the units
    struct { long long* num; unsigned long long* cw; float *tmp, *pair; double* qs; unsigned* mb; } L;
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, L, [&](Carver& c, auto& r) {
        r.num = c.take<long long>(n * sizeof(long long));
        r.cw = c.take<unsigned long long>(n * sizeof(unsigned long long));
        r.tmp = c.take<float>(n * sizeof(float));
        r.pair = c.take<float>(basic ? 2 * n * sizeof(float) : 0);
        r.qs = c.take<double>((size_t)batch * 2 * sizeof(double));
        r.mb = c.take<unsigned>((size_t)batch * sizeof(unsigned));
    });
    if (rc) return rc;
    const size_t sums = reinterpret_cast<char*>(L.tmp) - reinterpret_cast<char*>(L.num);
    HIP_TRY(ctx, hipMemsetAsync(L.num, 0, sums, ctx->stream));
    HIP_TRY(ctx, launch_qscale(noisy, (size_t)g.nvox, batch, data_exp, L.mb, L.qs, ctx->stream, ctx->status_dev));
    HIP_TRY(ctx, launch_stage(noisy, basic, keys, g, batch, ctx->dct, ctx->win_dev.as<float>(), thr, sigma2, L.qs,
                              L.num, L.cw, ctx->stream, ctx->stage, basic ? L.pair : nullptr, 0));
    HIP_TRY(ctx, launch_num_to_float(L.num, L.qs, num, (size_t)g.nvox, batch, ctx->stream));
    HIP_TRY(ctx, launch_den_from_corners(L.cw, L.tmp, den, g.nz, g.ny, g.nx, batch, ctx->win1d, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_normalize_dev(exabm4d_ctx* ctx, const float* num, const float* den, float* out,
                          size_t n, float clip_lo, float clip_hi) {
    if (!ctx || !num || !den || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_normalize(num, den, out, n, clip_lo, clip_hi, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_counts_from_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, float* out, size_t n, float offset) {
    if (!ctx || !in || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_counts_from_u16(in, out, n, offset, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_round_counts_f32_dev(exabm4d_ctx* ctx, const float* in, float* out, size_t n, float offset) {
    if (!ctx || !in || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_round_counts(in, out, nullptr, n, offset, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_normalize_u16_dev(exabm4d_ctx* ctx, const float* num, const float* den, uint16_t* out,
                              size_t n, float offset) {
    if (!ctx || !num || !den || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_normalize_u16(num, den, out, n, offset, ctx->stream));
    return EXABM4D_OK;
}

// Bracket one phase of a pipeline call with events when profiling is on.
struct PhaseTimer {
    exabm4d_ctx* ctx;
    int phase;
    PhaseTimer(exabm4d_ctx* c, int p) : ctx(c), phase(p) {
        if (ctx->profile) (void)hipEventRecord(ctx->ev[2 * phase], ctx->stream);
    }
    ~PhaseTimer() {
        if (ctx->profile) {
            (void)hipEventRecord(ctx->ev[2 * phase + 1], ctx->stream);
            ctx->ev_used[phase] = true;
        }
    }
};

// ---- zeroing of the 8-byte sums -------------------------------------------------------------------------------
// NUM and CW (16 bytes per voxel) are zeroed before every stage kernel: 2.7 ms per stage at 1024^3 when the
// memsets sit on the context's stream.  Block matching runs between the sums' last reader (the previous
// normalisation) and their next writer (the stage kernel), is bound by instruction issue and touches neither
// array: the memsets go to a second stream there -- zero_begin() after the last reader, zero_join() before the
// stage kernel -- and cost the step nothing.  Only where there is something to hide: below 2^25 voxels (0.1 ms
// of memsets) the two cross-stream dependencies cost more than they save (+15 us on a 64^3 patch's 1.8 ms).
static int zero_begin(exabm4d_ctx* ctx, long long* num, unsigned long long* cw, size_t n, hipStream_t s) {
    hipStream_t z = s;
    ctx->zero_on_side = ctx->zero_overlap && n >= ((size_t)1 << 25);
    if (ctx->zero_on_side) {
        HIP_TRY(ctx, hipEventRecord(ctx->side_ev[0], s));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->side_ev[0], 0));
        z = ctx->side;
    }
    HIP_TRY(ctx, hipMemsetAsync(num, 0, n * sizeof(long long), z));
    HIP_TRY(ctx, hipMemsetAsync(cw, 0, n * sizeof(unsigned long long), z));
    if (ctx->zero_on_side) HIP_TRY(ctx, hipEventRecord(ctx->side_ev[1], ctx->side));
    return EXABM4D_OK;
}
static int zero_join(exabm4d_ctx* ctx, hipStream_t s) {
    if (ctx->zero_on_side) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->side_ev[1], 0));
    ctx->zero_on_side = false;
    return EXABM4D_OK;
}

// ---- whole pipeline -----------------------------------------------------------------------------------------
static int run_pipeline(exabm4d_ctx* ctx, const VolGeom& g, int batch, float sigma, const exabm4d_params* p,
                        int stages, const PipeRun& run) {
    const float* noisy = run.noisy;
    uint16_t* const counts16 = run.counts16;
    const size_t n = (size_t)g.nvox * (size_t)batch;
    const BmPlan plan = bm_plan(g, batch, ctx->bm);           // one plan for both matching launches
    Carver c{ctx->scratch.as<char>()};
    PipeLayout L;
    pipe_layout(c, L, n, (size_t)g.nref * (size_t)batch, batch, stages, plan.carry_bytes);
    const auto [keys, num, basic, cw, tmp, pairvol, qs, maxbits, carry] = L;     // basic: only touched when stages >= 2

    const float thr = (float)((double)p->lambda_ht * (double)sigma);
    const float sigma2 = (float)((double)sigma * (double)sigma);
    hipStream_t s = ctx->stream;
    // what the first normalisation wrote besides `basic`: the Wiener stage's (noisy, basic) volume, the rounded counts
    NormWrote basic_wrote{hipSuccess, false, false};
    // stage 2 of a uint16 pipeline in the integer kernel?  Decided here because the first
    // normalisation then also writes the rounded estimate (into counts16's memory: stage 1 is done with it)
    const bool match_use16 = run.match_rounded && stages >= 2 &&
                             int_match_ok(ctx, p->c_match_wie, sigma, g, counts16, n, run.counts_offset);
    const NormSums sums{num, qs, tmp, g.nz, g.ny, g.nx, batch, ctx->win1d};
    if (ctx->profile)
        for (int i = 1; i < EXABM4D_PHASE_COUNT; i++) ctx->ev_used[i] = false;
    if ((run.in_scratch && !guarded_region_ok(ctx, noisy, n * sizeof(float))) ||
        (stages >= 2 && !guarded_region_ok(ctx, basic, n * sizeof(float))))
        return fail(ctx, EXABM4D_ERR_INVALID, "internal: guarded volume without mapped slack around it");

    {
        PhaseTimer t(ctx, EXABM4D_PHASE_ZERO_ACC_1);
        int rc = zero_begin(ctx, num, cw, n, s);
        if (rc) return rc;
        HIP_TRY(ctx, launch_qscale(noisy, (size_t)g.nvox, batch, run.data_exp, maxbits, qs, s, ctx->status_dev));
    }
    {
        PhaseTimer t(ctx, EXABM4D_PHASE_BLOCKMATCH_HT);
        const bool use16 = int_match_ok(ctx, p->c_match_ht, sigma, g, counts16, n, run.counts_offset);
        HIP_TRY(ctx, launch_blockmatch(noisy, g, batch, keymax_of(sigma, p->c_match_ht), keys, s,
                                       ctx->force_generic_bm, run.in_scratch, use16 ? counts16 : nullptr, plan,
                                       carry, ctx->status_dev));
    }
    {
        PhaseTimer t(ctx, EXABM4D_PHASE_STAGE_HT);
        int rc = zero_join(ctx, s);
        if (rc) return rc;
        HIP_TRY(ctx, launch_stage(noisy, nullptr, keys, g, batch, ctx->dct, ctx->win_dev.as<float>(), thr, sigma2, qs, num, cw,
                                  s, ctx->stage));
        HIP_TRY(ctx, launch_den_xy_from_corners(cw, tmp, g.nz, g.ny, g.nx, batch, ctx->win1d, s));
    }
    if (stages >= 2) {
        {
            PhaseTimer t(ctx, EXABM4D_PHASE_NORMALIZE_BASIC);
            // ... and, where it can, the Wiener stage's interleaved (noisy, basic) volume
            const NormSide side{ctx->stage.pairvol ? noisy : nullptr, pairvol, match_use16 ? counts16 : nullptr,
                                run.counts_offset};
            basic_wrote = launch_normalize_zconv(sums, NormOut::to_f32(basic), s, &side);
            HIP_TRY(ctx, basic_wrote.err);
        }
        {
            PhaseTimer t(ctx, EXABM4D_PHASE_ZERO_ACC_2);
            int rc = zero_begin(ctx, num, cw, n, s);
            if (rc) return rc;
        }
        {
            PhaseTimer t(ctx, EXABM4D_PHASE_BLOCKMATCH_WIE);
            const float* match_on = basic;
            const uint16_t* match16 = nullptr;
            int match_guarded = 1;
            if (run.match_rounded) {
                if (match_use16) {
                    if (!basic_wrote.round16)                            // (normally written by the normalisation)
                        HIP_TRY(ctx, launch_round_counts(basic, nullptr, counts16, n, run.counts_offset, s));
                    match16 = counts16;
                }
                // reference blocks at clamped grid positions (an extent - 8 that is no multiple of 4) go through
                // the one-wave kernel, which reads fp32: it needs the same counts as fp32
                const bool generic_too = ctx->force_generic_bm || g.gz != g.az || g.gy != g.ay || g.gx != g.ax;
                if (!match_use16 || generic_too) {
                    HIP_TRY(ctx, launch_round_counts(basic, tmp, nullptr, n, run.counts_offset, s));
                    match_on = tmp;
                    match_guarded = guarded_region_ok(ctx, tmp, n * sizeof(float)) ? 1 : 0;
                }
            }
            HIP_TRY(ctx, launch_blockmatch(match_on, g, batch, keymax_of(sigma, p->c_match_wie), keys,
                                           s, ctx->force_generic_bm, match_guarded, match16, plan, carry,
                                           ctx->status_dev));
        }
        {
            PhaseTimer t(ctx, EXABM4D_PHASE_STAGE_WIE);
            int rc = zero_join(ctx, s);
            if (rc) return rc;
            HIP_TRY(ctx, launch_stage(noisy, basic, keys, g, batch, ctx->dct, ctx->win_dev.as<float>(), thr, sigma2, qs, num, cw,
                                      s, ctx->stage, pairvol, basic_wrote.pair ? 1 : 0));
            HIP_TRY(ctx, launch_den_xy_from_corners(cw, tmp, g.nz, g.ny, g.nx, batch, ctx->win1d, s));
        }
    }
    {
        PhaseTimer t(ctx, EXABM4D_PHASE_NORMALIZE_OUT);
        HIP_TRY(ctx, launch_normalize_zconv(sums, run.out, s).err);
    }
    return EXABM4D_OK;
}

int exabm4d_denoise_f32_dev(exabm4d_ctx* ctx, const float* in, float* out, int nz, int ny, int nx,
                            int batch, float sigma, const exabm4d_params* p, int stages,
                            float clip_lo, float clip_hi) {
    VolGeom g;
    int rc = pipeline_checks(ctx, in, out, nz, ny, nx, batch, sigma, p, stages, g);
    if (rc) return rc;
    rc = ensure_scratch(ctx, pipe_bytes(ctx->bm, nz, ny, nx, batch, stages));
    if (rc) return rc;
    return run_pipeline(ctx, g, batch, sigma, p, stages,
                        PipeRun::f32(in, CALLERS_BUFFER, NormOut::to_f32_abi_clip(out, clip_lo, clip_hi)));
}

// The body of the two uint16 device entries: scratch, the forward pass (counts - offset and the uint16 shadow, or
// under pg the stabilisation) as phase COUNTS_FROM_U16, the pipeline.
static int run_u16_pipeline(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, const VolGeom& g, int batch,
                            float sigma, float offset, const PgDev* pg, const exabm4d_params* p, int stages) {
    const size_t n = (size_t)g.nvox * (size_t)batch;
    U16Scratch v;
    int rc = u16_pipe_scratch(ctx, g, batch, stages, v);
    if (rc) return rc;
    ctx->ev_used[EXABM4D_PHASE_COUNTS_FROM_U16] = false;
    {
        PhaseTimer t(ctx, EXABM4D_PHASE_COUNTS_FROM_U16);
        if (pg)
            HIP_TRY(ctx, launch_pg_forward_u16(*pg, in, v.f32, n, ctx->stream));
        else
            HIP_TRY(ctx, launch_counts_from_u16(in, v.f32, n, offset, ctx->stream, v.u16));
    }
    return run_pipeline(ctx, g, batch, sigma, p, stages,
                        pg ? PipeRun::stabilised_to_u16(v.f32, out, pg) : PipeRun::counts_to_u16(v, offset, out));
}

int exabm4d_denoise_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                            int nx, int batch, float sigma, float offset, const exabm4d_params* p,
                            int stages) {
    VolGeom g;
    int rc = pipeline_checks(ctx, in, out, nz, ny, nx, batch, sigma, p, stages, g);
    if (rc) return rc;
    rc = check_offset(ctx, offset);
    if (rc) return rc;
    return run_u16_pipeline(ctx, in, out, g, batch, sigma, offset, nullptr, p, stages);
}

// Under Poisson-Gaussian noise: counts -> D (unit sigma) -> the fp32 pipeline at sigma 1 -> the
// inverse, fused into the last normalisation -> counts.  The scratch is the uint16 pipelines' (the uint16 shadow
// stays unused: both matching passes are the float kernels').
int exabm4d_denoise_pg_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny, int nx,
                               int batch, const exabm4d_pg_noise* noise, const exabm4d_params* p, int stages) {
    int rc = bm4d_checks(ctx, in, out, 1.0f, p, stages);
    if (rc) return rc;
    PgDev pg;
    rc = pg_entry(ctx, noise, pg);
    if (rc) return rc;
    VolGeom g;
    rc = geom_on_device(ctx, nz, ny, nx, batch, g);
    if (!rc) rc = ensure_window(ctx, (double)p->kaiser_beta);
    if (rc) return rc;
    return run_u16_pipeline(ctx, in, out, g, batch, 1.0f, 0.0f, &pg, p, stages);
}

int exabm4d_gat_forward_u16_dev(exabm4d_ctx* ctx, const exabm4d_pg_noise* noise, const uint16_t* in, float* out,
                                size_t n) {
    if (!ctx || !in || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    PgDev pg;
    int rc = pg_entry(ctx, noise, pg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_pg_forward_u16(pg, in, out, n, ctx->stream));
    return EXABM4D_OK;
}

int exabm4d_gat_inverse_u16_dev(exabm4d_ctx* ctx, const exabm4d_pg_noise* noise, const float* in, uint16_t* out,
                                size_t n) {
    if (!ctx || !in || !out) return fail(ctx, EXABM4D_ERR_INVALID, "NULL argument");
    PgDev pg;
    int rc = pg_entry(ctx, noise, pg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_pg_inverse_u16(pg, in, out, n, ctx->stream));
    return EXABM4D_OK;
}

// Chunk-local mode: every chunk (core + halo, the halo cut off where the buffer ends) is denoised
// in isolation, batches of equally shaped chunks per pipeline run; only the cores are written.
// pg == NULL: the uint16 pipeline at (sigma, offset); else the stabilised pipeline at sigma 1.
// The arguments have been checked by the entry points below.
static int chunked_on_device(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny, int nx, int zc0,
                             int zc1, int chunk, int halo, float sigma, float offset, const PgDev* pg,
                             const exabm4d_params* p, int stages) {
    int rc = EXABM4D_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ensure_window(ctx, (double)p->kaiser_beta);
    if (rc) return rc;
    const std::vector<ChunkRun> runs[3] = {chunk_runs(nz, zc0, zc1, chunk, halo),
                                           chunk_runs(ny, 0, ny, chunk, halo),
                                           chunk_runs(nx, 0, nx, chunk, halo)};
    for (int a = 0; a < 3; a++)
        for (const ChunkRun& r : runs[a])
            if (r.e + r.lo + r.hi < 8)
                return fail(ctx, EXABM4D_ERR_INVALID, "chunked: a padded chunk would be thinner than one block (8)");
    ctx->ev_used[EXABM4D_PHASE_COUNTS_FROM_U16] = false;
    const ChunkMap map{offset, pg};
    for (const ChunkRun& rz : runs[0])
        for (const ChunkRun& ry : runs[1])
            for (const ChunkRun& rx : runs[2]) {
                ChunkBatch cb;
                cb.nz = nz; cb.ny = ny; cb.nx = nx;
                cb.z0 = zc0 + rz.i0 * chunk; cb.y0 = ry.i0 * chunk; cb.x0 = rx.i0 * chunk;
                cb.cz = cb.cy = cb.cx = chunk;
                cb.ez = rz.e; cb.ey = ry.e; cb.ex = rx.e;
                cb.lz = rz.lo; cb.ly = ry.lo; cb.lx = rx.lo;
                cb.pz = rz.e + rz.lo + rz.hi; cb.py = ry.e + ry.lo + ry.hi; cb.px = rx.e + rx.lo + rx.hi;
                cb.sgy = ry.count; cb.sgx = rx.count;
                cb.out_z0 = zc0;
                const long long nchunks = (long long)rz.count * ry.count * rx.count;
                const size_t per = pipe_bytes(ctx->bm, cb.pz, cb.py, cb.px, 1, stages) +
                                   align256((size_t)cb.pz * cb.py * cb.px * (sizeof(float) + sizeof(uint16_t)));
                long long bmax = (long long)(((size_t)ctx->chunk_budget_mb << 20) / per);
                if (bmax < 1) bmax = 1;
                if (bmax > 65535) bmax = 65535;
                for (long long first = 0; first < nchunks; first += bmax) {
                    const int count = (int)std::min<long long>(bmax, nchunks - first);
                    cb.first = (int)first;
                    cb.count = count;
                    VolGeom g;
                    rc = make_geom(ctx, cb.pz, cb.py, cb.px, count, g);
                    if (rc) return rc;
                    U16Scratch v;
                    rc = u16_pipe_scratch(ctx, g, count, stages, v);
                    if (rc) return rc;
                    // under pg the chunks are stabilised volumes: the fp32 pipeline at sigma 1, in place
                    HIP_TRY(ctx, launch_chunk_gather(in, cb, map, v.f32, ctx->stream, pg ? nullptr : v.u16));
                    rc = run_pipeline(ctx, g, count, sigma, p, stages,
                                      pg ? PipeRun::f32(v.f32, IN_SCRATCH, NormOut::to_f32(v.f32))
                                         : PipeRun::counts_in_place(v, offset));
                    if (rc) return rc;
                    HIP_TRY(ctx, launch_chunk_scatter(v.f32, cb, map, out, ctx->stream));
                }
            }
    return EXABM4D_OK;
}

int exabm4d_denoise_chunked_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                    int nx, int zc0, int zc1, int chunk, int halo, float sigma,
                                    float offset, const exabm4d_params* p, int stages) {
    int rc = chunk_checks(ctx, in, out, nz, ny, nx, chunk, halo, sigma, p, stages);
    if (rc) return rc;
    if (zc0 < 0 || zc1 > nz || zc0 >= zc1) return fail(ctx, EXABM4D_ERR_INVALID, "chunked: bad core plane range");
    rc = check_offset(ctx, offset);
    if (rc) return rc;
    return chunked_on_device(ctx, in, out, nz, ny, nx, zc0, zc1, chunk, halo, sigma, offset, nullptr, p, stages);
}

int exabm4d_denoise_pg_chunked_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                       int nx, int zc0, int zc1, int chunk, int halo,
                                       const exabm4d_pg_noise* noise, const exabm4d_params* p, int stages) {
    int rc = chunk_checks(ctx, in, out, nz, ny, nx, chunk, halo, 1.0f, p, stages);
    if (rc) return rc;
    if (zc0 < 0 || zc1 > nz || zc0 >= zc1) return fail(ctx, EXABM4D_ERR_INVALID, "chunked: bad core plane range");
    PgDev pg;
    rc = pg_entry(ctx, noise, pg);
    if (rc) return rc;
    return chunked_on_device(ctx, in, out, nz, ny, nx, zc0, zc1, chunk, halo, 1.0f, pg.off, &pg, p, stages);
}

// ---- chunk-local mode, host volume streamed through the device ------------------------------------
// A host volume of any size (BASELINE config 4's tile is 64 GiB of uint16) goes through the device one
// LAYER of chunks at a time: planes [k chunk - halo, (k + 1) chunk + halo) up, cores down.  Two
// device windows and two result buffers; an uploader and a downloader thread (plain copies on their
// own streams: the host side of a pageable copy blocks, so each direction gets a thread) run one layer
// ahead of / behind exabm4d_denoise_chunked_u16_dev on the context's stream.  Chunks are independent
// units, so the result is the one-call result of exabm4d_denoise_chunked_u16_dev on the whole volume.
namespace {
struct StreamedLayers {
    std::mutex m;
    std::condition_variable cv;
    int uploaded = 0;       // layers whose window is on the device
    int enqueued = 0;       // layers whose compute has been enqueued (comp_ev[k & 1] recorded)
    int downloaded = 0;     // layers whose cores are back in the caller's array
    bool failed = false;
    std::string err;

    void advance(int StreamedLayers::*field) {
        { std::lock_guard<std::mutex> l(m); (this->*field)++; }
        cv.notify_all();
    }
    bool wait_for(int StreamedLayers::*field, int value) {      // false: somebody failed
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return failed || this->*field >= value; });
        return !failed;
    }
    void fail_with(const std::string& what) {
        { std::lock_guard<std::mutex> l(m); if (!failed) { failed = true; err = what; } }
        cv.notify_all();
    }
};
}  // namespace

// pg == NULL: (sigma, offset) through chunked_on_device's uint16 pipeline; else the stabilised one.  Arguments
// checked by the entry points below.
static int chunked_from_host(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny, int nx, int chunk,
                             int halo, float sigma, float offset, const PgDev* pg, const exabm4d_params* p,
                             int stages) {
    int rc = EXABM4D_OK;
    {   // the downloads of early layers would overwrite planes that later layers still have to upload
        const size_t bytes = (size_t)nz * (size_t)ny * (size_t)nx * sizeof(uint16_t);
        const char *a = reinterpret_cast<const char*>(in), *b = reinterpret_cast<const char*>(out);
        if (a < b + bytes && b < a + bytes)
            return fail(ctx, EXABM4D_ERR_INVALID, "streamed chunk mode: input and output arrays overlap");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int layers = (nz + chunk - 1) / chunk;
    const size_t plane = (size_t)ny * (size_t)nx;
    const int wmax = std::min(nz, chunk + 2 * halo), cmax = std::min(nz, chunk);
    const int device = ctx->device;

    uint16_t* win[2] = {nullptr, nullptr};
    uint16_t* res[2] = {nullptr, nullptr};
    hipStream_t s_up = nullptr, s_down = nullptr;
    hipEvent_t comp_ev[2] = {nullptr, nullptr};
    const int nbuf = layers > 1 ? 2 : 1;
    auto release = [&]() {
        for (int i = 0; i < 2; i++) {
            if (win[i]) (void)hipFree(win[i]);
            if (res[i]) (void)hipFree(res[i]);
            if (comp_ev[i]) (void)hipEventDestroy(comp_ev[i]);
        }
        if (s_up) (void)hipStreamDestroy(s_up);
        if (s_down) (void)hipStreamDestroy(s_down);
    };
    hipError_t e = hipSuccess;
    for (int i = 0; i < nbuf && e == hipSuccess; i++) {
        e = hipMalloc((void**)&win[i], (size_t)wmax * plane * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc((void**)&res[i], (size_t)cmax * plane * sizeof(uint16_t));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&comp_ev[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s_down, hipStreamNonBlocking);
    if (e != hipSuccess) {
        release();
        return fail_hip(ctx, e, "streamed chunk mode: device windows / streams");
    }

    StreamedLayers st;
    auto window_of = [&](int k, int& w0, int& w1, int& c0, int& c1) {
        c0 = k * chunk;
        c1 = std::min(nz, c0 + chunk);
        w0 = std::max(0, c0 - halo);
        w1 = std::min(nz, c1 + halo);
    };
    auto upload_layers = [&]() {
        if (hipSetDevice(device) != hipSuccess) return st.fail_with("uploader: hipSetDevice");
        for (int k = 0; k < layers; k++) {
            if (k >= 2) {       // window k & 1 was read by layer k - 2
                if (!st.wait_for(&StreamedLayers::enqueued, k - 1)) return;
                if (hipEventSynchronize(comp_ev[k & 1]) != hipSuccess) return st.fail_with("uploader: hipEventSynchronize");
            }
            int w0, w1, c0, c1;
            window_of(k, w0, w1, c0, c1);
            hipError_t r = hipMemcpyAsync(win[k & 1], in + (size_t)w0 * plane, (size_t)(w1 - w0) * plane * sizeof(uint16_t),
                                          hipMemcpyHostToDevice, s_up);
            if (r == hipSuccess) r = hipStreamSynchronize(s_up);
            if (r != hipSuccess) return st.fail_with(std::string("upload of a chunk layer: ") + hipGetErrorString(r));
            st.advance(&StreamedLayers::uploaded);
        }
    };
    auto download_layers = [&]() {
        if (hipSetDevice(device) != hipSuccess) return st.fail_with("downloader: hipSetDevice");
        for (int k = 0; k < layers; k++) {
            if (!st.wait_for(&StreamedLayers::enqueued, k + 1)) return;
            int w0, w1, c0, c1;
            window_of(k, w0, w1, c0, c1);
            hipError_t r = hipEventSynchronize(comp_ev[k & 1]);
            if (r == hipSuccess)
                r = hipMemcpyAsync(out + (size_t)c0 * plane, res[k & 1], (size_t)(c1 - c0) * plane * sizeof(uint16_t),
                                   hipMemcpyDeviceToHost, s_down);
            if (r == hipSuccess) r = hipStreamSynchronize(s_down);
            if (r != hipSuccess) return st.fail_with(std::string("download of a chunk layer: ") + hipGetErrorString(r));
            st.advance(&StreamedLayers::downloaded);
        }
    };
    // no C++ exception may cross the C boundary: a thread that cannot be started is an error code
    std::thread uploader, downloader;
    try {
        uploader = std::thread(upload_layers);
        downloader = std::thread(download_layers);
    } catch (const std::exception& ex) {
        st.fail_with(std::string("cannot start a copy thread: ") + ex.what());
        if (uploader.joinable()) uploader.join();
        release();
        return fail(ctx, EXABM4D_ERR_NOMEM, "streamed chunk mode: " + st.err);
    }

    std::string compute_err;
    for (int k = 0; k < layers; k++) {
        // the window is up; the result buffer k & 1 (layer k - 2's) has been fetched
        if (!st.wait_for(&StreamedLayers::uploaded, k + 1) || !st.wait_for(&StreamedLayers::downloaded, k - 1)) break;
        int w0, w1, c0, c1;
        window_of(k, w0, w1, c0, c1);
        rc = chunked_on_device(ctx, win[k & 1], res[k & 1], w1 - w0, ny, nx, c0 - w0, c1 - w0, chunk, halo, sigma,
                               offset, pg, p, stages);
        hipError_t r = rc ? hipSuccess : hipEventRecord(comp_ev[k & 1], ctx->stream);
        if (rc || r != hipSuccess) {
            compute_err = rc ? ctx->err : std::string("hipEventRecord: ") + hipGetErrorString(r);
            if (!rc) rc = EXABM4D_ERR_HIP;
            st.fail_with(compute_err);
            break;
        }
        st.advance(&StreamedLayers::enqueued);
    }
    uploader.join();
    downloader.join();
    (void)hipStreamSynchronize(ctx->stream);
    release();
    if (st.failed) return fail(ctx, rc ? rc : EXABM4D_ERR_HIP, "streamed chunk mode: " + st.err);
    return check_async_status(ctx);
}

int exabm4d_denoise_chunked_u16_host(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                     int nx, int chunk, int halo, float sigma, float offset,
                                     const exabm4d_params* p, int stages) {
    int rc = chunk_checks(ctx, in, out, nz, ny, nx, chunk, halo, sigma, p, stages);
    if (!rc) rc = check_offset(ctx, offset);
    if (rc) return rc;
    return chunked_from_host(ctx, in, out, nz, ny, nx, chunk, halo, sigma, offset, nullptr, p, stages);
}

int exabm4d_denoise_pg_chunked_u16_host(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                        int nx, int chunk, int halo, const exabm4d_pg_noise* noise,
                                        const exabm4d_params* p, int stages) {
    int rc = chunk_checks(ctx, in, out, nz, ny, nx, chunk, halo, 1.0f, p, stages);
    if (rc) return rc;
    PgDev pg;
    rc = pg_entry(ctx, noise, pg);
    if (rc) return rc;
    return chunked_from_host(ctx, in, out, nz, ny, nx, chunk, halo, 1.0f, pg.off, &pg, p, stages);
}

// A large batch goes through the device in sub-batches of about 2^26 voxels, double-buffered: while sub-batch k
// is computed, the results of k - 1 come down and the input of k + 1 goes up on a copy stream of the context's
// (the host side of a pageable copy blocks, which is all the ordering this thread needs; the device side is
// ordered by events).  Every volume carries its own fixed-point unit, so the cut changes no bit.  1000 patches
// of 64^3, host to host: 245 -> see DESIGN.md 8a; the scratch is that of one sub-batch, not of the batch.
static constexpr size_t HOST_SUB_VOXELS = (size_t)1 << 26;
static int denoise_f32_host_pipelined(exabm4d_ctx* ctx, const float* in, float* out, int nz, int ny, int nx,
                                      int batch, int sub, float sigma, const exabm4d_params* p, int stages,
                                      float clip_lo, float clip_hi, unsigned* fired) {
    VolGeom g;
    int rc = make_geom(ctx, nz, ny, nx, sub, g);
    if (rc) return rc;
    const size_t nv = (size_t)g.nvox, nsubvox = nv * (size_t)sub;
    const size_t pipe = pipe_bytes(ctx->bm, nz, ny, nx, sub, stages);
    struct { float* buf[2]; } L;         // behind run_pipeline's regions, each followed by GUARD_BYTES
    rc = carve(ctx, ctx->scratch, GUARD_BYTES, L, [&](Carver& c, auto& r) {
        c.take(pipe);
        for (float*& b : r.buf) b = c.take<float>(nsubvox * sizeof(float) + GUARD_BYTES);
    });
    if (rc) return rc;
    if (!ctx->copy_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 3; i++) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->copy_ev[i], hipEventDisableTiming));
    }
    float* const* buf = L.buf;
    hipStream_t cs = ctx->copy_stream, s = ctx->stream;
    const int nsub = (batch + sub - 1) / sub;
    auto count_of = [&](int k) { return std::min(sub, batch - k * sub); };
    // the buffers' last users were earlier calls on the compute stream
    HIP_TRY(ctx, hipEventRecord(ctx->copy_ev[2], s));
    HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->copy_ev[2], 0));
    HIP_TRY(ctx, hipMemcpyAsync(buf[0], in, nv * count_of(0) * sizeof(float), hipMemcpyHostToDevice, cs));
    for (int k = 0; k < nsub; k++) {
        const int cnt = count_of(k);
        VolGeom gk = g;
        if (cnt != sub) {
            rc = make_geom(ctx, nz, ny, nx, cnt, gk);
            if (rc) return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->copy_ev[2], cs));                     // input k is up
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->copy_ev[2], 0));
        rc = run_pipeline(ctx, gk, cnt, sigma, p, stages,
                          PipeRun::f32(buf[k & 1], IN_SCRATCH, NormOut::to_f32_abi_clip(buf[k & 1], clip_lo, clip_hi)));
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->copy_ev[k & 1], s));                  // result k is ready
        if (k >= 1) {                                                          // result k - 1 down, under compute k
            HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->copy_ev[(k - 1) & 1], 0));
            HIP_TRY(ctx, hipMemcpyAsync(out + (size_t)(k - 1) * nsubvox, buf[(k - 1) & 1],
                                        nv * count_of(k - 1) * sizeof(float), hipMemcpyDeviceToHost, cs));
        }
        if (k + 1 < nsub)                                                      // input k + 1 up, into the buffer just emptied
            HIP_TRY(ctx, hipMemcpyAsync(buf[(k + 1) & 1], in + (size_t)(k + 1) * nsubvox,
                                        nv * count_of(k + 1) * sizeof(float), hipMemcpyHostToDevice, cs));
    }
    HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->copy_ev[(nsub - 1) & 1], 0));
    HIP_TRY(ctx, hipMemcpyAsync(out + (size_t)(nsub - 1) * nsubvox, buf[(nsub - 1) & 1],
                                nv * count_of(nsub - 1) * sizeof(float), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return check_async_status(ctx, fired);
}

// A host run is repeated, once and in one piece, only when the carry's wait ran out (bit 0) in a run that had the
// carry on (check_async_status has now switched it off); any other error, bit 1 included, is returned as is.
static bool repeat_without_carry(unsigned fired, bool carry_was_on) { return (fired & 1u) && carry_was_on; }

// The host batch entries' body: the batch lies in `pieces` host arrays of `per_piece` voxels.  `out[i]` may be
// `in[i]`: the results go to the host only once the run is known to be good, and a repeat reads `in` again.
static int host_batch(exabm4d_ctx* ctx, const float* const* in, float* const* out, int pieces, size_t per_piece,
                      const VolGeom& g, int batch, float sigma, const exabm4d_params* p, int stages, float clip_lo,
                      float clip_hi) {
    const size_t n = (size_t)g.nvox * (size_t)batch;
    int rc = EXABM4D_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        const bool carry_was_on = ctx->bm.carry != 0;
        const size_t pipe = pipe_bytes(ctx->bm, g.nz, g.ny, g.nx, batch, stages);
        float* vol;          // behind run_pipeline's regions
        rc = carve(ctx, ctx->scratch, GUARD_BYTES, vol, [&](Carver& c, float*& r) {
            c.take(pipe);
            r = c.take<float>(n * sizeof(float));
        });
        if (rc) return rc;
        for (int i = 0; i < pieces; i++)
            HIP_TRY(ctx, hipMemcpyAsync(vol + (size_t)i * per_piece, in[i], per_piece * sizeof(float),
                                        hipMemcpyHostToDevice, ctx->stream));
        rc = run_pipeline(ctx, g, batch, sigma, p, stages,
                          PipeRun::f32(vol, IN_SCRATCH, NormOut::to_f32_abi_clip(vol, clip_lo, clip_hi)));
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        unsigned fired = 0;
        rc = check_async_status(ctx, &fired);
        if (rc == EXABM4D_OK) {
            for (int i = 0; i < pieces; i++)
                HIP_TRY(ctx, hipMemcpyAsync(out[i], vol + (size_t)i * per_piece, per_piece * sizeof(float),
                                            hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return EXABM4D_OK;
        }
        if (!repeat_without_carry(fired, carry_was_on)) return rc;
    }
    return rc;
}

int exabm4d_denoise_f32_host(exabm4d_ctx* ctx, const float* in, float* out, int nz, int ny, int nx,
                             int batch, float sigma, const exabm4d_params* p, int stages,
                             float clip_lo, float clip_hi) {
    VolGeom g;
    int rc = pipeline_checks(ctx, in, out, nz, ny, nx, batch, sigma, p, stages, g);
    if (rc) return rc;
    // Large batches of volumes: sub-batches with the copies under the kernels.  Not in place (a repeated run
    // must find its input), not while a debug option wants to see one launch.
    const size_t per = std::max<size_t>(1, HOST_SUB_VOXELS / (size_t)g.nvox);
    if (ctx->host_pipeline && in != out && batch >= 2 && (size_t)batch >= 2 * per && per <= 65535) {
        const bool carry_was_on = ctx->bm.carry != 0;
        unsigned fired = 0;
        rc = denoise_f32_host_pipelined(ctx, in, out, nz, ny, nx, batch, (int)per, sigma, p, stages, clip_lo,
                                        clip_hi, &fired);
        if (rc != EXABM4D_OK && ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);   // nothing of it left in flight
        if (rc == EXABM4D_OK || !repeat_without_carry(fired, carry_was_on)) return rc;
        // the carry's wait ran out somewhere (it is off now): once more, in one piece
    }
    return host_batch(ctx, &in, &out, 1, (size_t)g.nvox * (size_t)batch, g, batch, sigma, p, stages, clip_lo,
                      clip_hi);
}

// The same for a batch whose volumes lie anywhere in host memory (the broker's shape: every caller's patch in
// its own shared-memory segment): in[i] / out[i] per volume, out[i] may be in[i].
int exabm4d_denoise_f32_host_v(exabm4d_ctx* ctx, const float* const* in, float* const* out, int nz, int ny,
                               int nx, int batch, float sigma, const exabm4d_params* p, int stages,
                               float clip_lo, float clip_hi) {
    VolGeom g;
    int rc = pipeline_checks(ctx, in, out, nz, ny, nx, batch, sigma, p, stages, g);
    if (rc) return rc;
    for (int b = 0; b < batch; b++)
        if (!in[b] || !out[b]) return fail(ctx, EXABM4D_ERR_INVALID, "NULL volume pointer");
    return host_batch(ctx, in, out, batch, (size_t)g.nvox, g, batch, sigma, p, stages, clip_lo, clip_hi);
}

}  // extern "C"
