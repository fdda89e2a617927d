/*
 * exabm4d.h -- C-ABI of libexabm4d.so (MI355X / gfx950 native BM4D denoise + intensity
 * transform + overlap-tile stitching hot path for ExaSPIM uint16 volumes).
 *
 * This is the drop-in boundary for the hot path of
 * AllenNeuralDynamics/aind-exaspim-image-compression.  The reference is pure Python; the
 * arithmetic on its hot path is reached through these interfaces, each of which one entry
 * point below replaces (paths relative to the reference checkout, src/aind_exaspim_image_compression/):
 *
 *   bm4d(raw, sigma)                      machine_learning/data_handling.py:332, :926 ; evaluate.py:202
 *   np.clip(teacher, 0, max_count)        machine_learning/data_handling.py:333, :927
 *   read_counts (u16 -> f32 - offset)     machine_learning/data_handling.py:337-354
 *   IntensityTransform.forward            machine_learning/transforms.py:113-129, :244-259, :332-348, :398-401
 *   IntensityTransform.inverse[_float]    machine_learning/transforms.py:131-152, :261-285, :350-371, :403-411
 *   predict(): patch gather / pad         inference.py:153-174, :178-199, :202-226
 *   predict(): accumulate / normalise     inference.py:81-116
 *   estimate_offset (np.percentile)       machine_learning/transforms.py:414-438
 *   ssim3D, compute_mae, compute_lmax     utils/img_util.py:953-1050
 *   evaluate_example and its parts        machine_learning/metrics.py:306-424
 *   compute_cratio's codec.encode loop    utils/img_util.py:401-441 (codec: evaluate.py:40)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, POD structs whose first field is their own sizeof
 *     (ABI evolution).  No allocation is returned across the ABI except through
 *     exabm4d_malloc/exabm4d_free (thin hipMalloc wrappers for hosts without a device
 *     allocator of their own).
 *   - Every function returns 0 on success or a negative exabm4d_status; a message is available
 *     from exabm4d_last_error().  No C++ exception crosses the boundary.
 *   - "_dev" functions take DEVICE pointers and enqueue on the context's stream without
 *     synchronising; "_host" functions take HOST pointers, copy in/out and synchronise.
 *   - Volumes are C-contiguous [z][y][x]; a batch is `batch` such volumes back to back.
 *   - A context belongs to one (process, device); create it after fork(), never before
 *     (the reference calls bm4d from forked ProcessPoolExecutor workers, scripts/precompute.py:215).
 *   - The BM4D algorithm is the specification frozen in DESIGN.md section 3 (the reference's
 *     own BM4D is the closed third-party wheel bm4d==4.2.5, uv.lock:387-400; parity with it is
 *     unpinned -- see DESIGN.md).
 */
#ifndef EXABM4D_H
#define EXABM4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXABM4D_VERSION 400 /* additive within 400: + exabm4d_pg_noise, exabm4d_denoise_pg_u16_dev, exabm4d_denoise_pg_chunked_u16_dev / _host, exabm4d_gat_forward_u16_dev, exabm4d_gat_inverse_u16_dev (denoising under Poisson-Gaussian noise); + exabm4d_dctq_ladder_errors_dev, exabm4d_bounded_volume_bound, exabm4d_bounded_encode_dev, exabm4d_bounded_decode_dev (error-bounded lossy chunk codec); + exabm4d_block_bounded_volume_bound, exabm4d_block_bounded_steps_dev, exabm4d_block_bounded_encode_dev, exabm4d_block_bounded_decode_dev (error-bounded codec with a step per 8^3 block and a per-voxel bound); + exabm4d_block_bounded_steps_tab_dev, exabm4d_block_bounded_encode_tab_dev (that codec's bound from a table of the voxel's value); + exabm4d_foreground_masks_dev, exabm4d_binary_dilate_dev, exabm4d_gaussian_filter3d_dev, exabm4d_label_set_dev, exabm4d_segment_stats_dev (patch-cache masks and coherence gate); + exabm4d_groupnorm_lrelu_ndhwc_dt_dev, exabm4d_maxpool2_ndhwc_dt_dev, exabm4d_upsample2_trilinear_ndhwc_dt_dev (fp16 / bf16 BM4DNet kernels); 0.4.0 (round 4): order-independent aggregation -- exabm4d_stage_dev takes data_exp and WRITES num / den, options "stage_pairs" / "stage_quads" / "fuse_den_z" are gone, the stage / block-matching options are per context; 0.3.2: + exabm4d_blockmatch_plan, option "stage_strip"; 0.3.1: + exabm4d_denoise_chunked_u16_host, options "bm_carry" / "bm_xcd_mode"; 0.3.0: EXAC v2 coder, exabm4d_codec_decode_dev takes in_bytes (round 3) */

typedef enum exabm4d_status {
    EXABM4D_OK = 0,
    EXABM4D_ERR_INVALID = -1,     /* bad argument (NULL pointer, dims < 8, bad struct size ...) */
    EXABM4D_ERR_UNSUPPORTED = -2, /* profile value outside what the kernels implement          */
    EXABM4D_ERR_HIP = -3,         /* a HIP runtime call failed (message has hipGetErrorString)  */
    EXABM4D_ERR_NOMEM = -4,       /* device scratch allocation failed                            */
    EXABM4D_ERR_NODEVICE = -5     /* no usable gfx950 device                                     */
} exabm4d_status;

/* BM4D profile.  Defaults (exabm4d_default_params) are BASELINE.json's parameter contract:
 * block 8^3, step 4, search window 11^3, groups of <= 16, 3-D DCT + Haar, lambda 2.7. */
typedef struct exabm4d_params {
    uint32_t size;        /* = sizeof(exabm4d_params)                                    */
    int32_t block;        /* cubic block edge; only 8 is implemented                      */
    int32_t step;         /* reference-block grid step; only 4                            */
    int32_t search;       /* search window edge (displacements -5..5); only 11            */
    int32_t max_group;    /* blocks per group, power of two <= 16; only 16               */
    float lambda_ht;      /* hard threshold = lambda_ht * sigma                           */
    float c_match_ht;     /* stage-1 match threshold: mean sq. diff <= c_match_ht*sigma^2 */
    float c_match_wie;    /* stage-2 match threshold (on the basic estimate)              */
    float kaiser_beta;    /* aggregation window, separable Kaiser(8, beta); 0 => all ones */
} exabm4d_params;

/* Intensity transform descriptor (machine_learning/transforms.py).  `kind` selects the base
 * transform; `wrapped` != 0 composes OffsetTransform(base, wrap_offset) around it
 * (transforms.py:374-411).  All parameters are the Python floats of the reference object;
 * the kernels round them to fp32 exactly where numpy does. */
enum { EXABM4D_TF_ASINH = 0, EXABM4D_TF_ANSCOMBE = 1, EXABM4D_TF_LINEAR = 2 };
typedef struct exabm4d_transform {
    uint32_t size;        /* = sizeof(exabm4d_transform) */
    int32_t kind;         /* EXABM4D_TF_*                */
    int32_t wrapped;      /* 0/1: OffsetTransform wrapper */
    int32_t reserved;
    double wrap_offset;   /* OffsetTransform.offset       */
    double max_count;     /* clamp of inverse(); for a wrapper: base.max_count */
    double offset;        /* asinh.offset / anscombe.offset                    */
    double scale;         /* asinh.scale                                        */
    double norm;          /* asinh._norm / anscombe._norm (python float)        */
    double gain;          /* anscombe.gain                                      */
    double read_noise;    /* anscombe.read_noise                                */
    double c_inv;         /* anscombe._c_inv (1/8 or 3/8)                       */
    double mn, mx, clip;  /* linear                                             */
} exabm4d_transform;

typedef struct exabm4d_ctx exabm4d_ctx;

/* ---- library / context ------------------------------------------------------------------ */
int exabm4d_version(void);
/* Message of the last failing call on this thread (ctx may be NULL). Never NULL. */
const char* exabm4d_last_error(const exabm4d_ctx* ctx);
/* Number of HIP devices visible (no context needed; does not initialise a device). */
int exabm4d_device_count(void);
int exabm4d_create(int device, exabm4d_ctx** out);
int exabm4d_destroy(exabm4d_ctx* ctx);
/* Enqueue on an existing hipStream_t, e.g. torch.cuda.current_stream().cuda_stream.  The handle
 * is used as given: NULL is the HIP null (legacy default) stream, which is what PyTorch's default
 * stream is.  exabm4d_reset_stream returns to the context's private non-blocking stream. */
int exabm4d_set_stream(exabm4d_ctx* ctx, void* hip_stream);
int exabm4d_reset_stream(exabm4d_ctx* ctx);
int exabm4d_sync(exabm4d_ctx* ctx);
int exabm4d_default_params(exabm4d_params* p);
/* Diagnostic switches. "force_generic_bm" = 1 routes every reference block through the
 * one-wave-per-block matching kernel (normally used only for grid points that are not a
 * multiple of 4); the parity tests use it to check the two kernels against each other.
 * "bm_guarded_copy" = 1 makes exabm4d_blockmatch_dev match on a copy of the volume inside the
 * library's scratch allocation, the way the exabm4d_denoise_* pipelines do (x-edge tiles then
 * stream their planes by LDS-DMA without clamping); for the parity tests.
 * Round 3: "codec_version" = 1 | 2 (default 2): the EXAC format exabm4d_codec_encode_dev writes (the
 * option is per context, not per call: do not switch it from two threads of one context);
 * "stage_pairvol" = 0 makes the Wiener kernel gather its two volumes separately (default 1: one
 * interleaved volume);
 * "bm_int" = 0 keeps the uint16 pipelines' stage-1 matching on the float kernel; "stage_chunks",
 * "chunk_budget_mb", "profile": z chunks of the stage kernels (0 = automatic), scratch budget of the
 * chunk-local mode, per-phase HIP events for exabm4d_profile_read.  "bm_carry" = 0 | 1 | 2 (default 1):
 * block matching's tiles hand their top cell layer to the tile above through device memory, eight
 * reference layers per tile instead of seven (1: where it saves a tile per column and the launch is large
 * enough, 2: wherever a column has two tiles; needs 744 KB of the context's scratch per tile column; tables
 * are identical).  A tile waits for the tile below it; workgroups take their tiles by ticket,
 * so the wait always ends, and it is bounded besides: should it ever run out, the kernel raises a status word
 * instead of hanging, the next synchronising call (exabm4d_sync, exabm4d_memcpy_d2h, *_host, ...) returns
 * EXABM4D_ERR_HIP, and the carry is off for that context from then on (exabm4d_denoise_f32_host repeats its
 * run without the carry by itself).  "bm_carry_fault" = 1 (debug) makes every such wait count as run out; "bm_layers" = 0 | 8 | 12 (default 0):
 * cell layers per tile of the integer block-matching kernel, 0 = 12 for large volumes in slab order with the carry, else 8
 * (tables are identical; any other value is EXABM4D_ERR_INVALID); "bm_xcd_mode" = 0 | 1 | n (default 2): workgroup order of
 * block matching; "host_pipeline" = 0 | 1 (default 1): exabm4d_denoise_f32_host cuts batches of >= 2^27 voxels
 * into sub-batches and copies under the kernels; "zero_overlap" = 0 | 1 (default 1): the 8-byte sums are zeroed on a second
 * stream of the context's, under the block matching that precedes each stage kernel, instead of in line
 * (DESIGN.md 5.3); "stage_strip" = 0 | n (default 3): tile-column order of the stage
 * kernels (0 = raster, n = strips of n tile rows; the same results, bit for bit: the sums are integers).
 * Every option belongs to the context it is set on (round 4; rounds 1-3 kept some in process globals). */
int exabm4d_set_option(exabm4d_ctx* ctx, const char* name, int value);
/* With option "profile" = 1 every exabm4d_denoise_* call brackets each of its kernel launches
 * with HIP events on the context's stream.  exabm4d_profile_read waits for the last call and
 * returns its per-phase durations in milliseconds, in EXABM4D_PHASE_* order (0 for a phase the
 * call did not run); returns the number of phases written (<= max_phases) or a negative status. */
enum {
    EXABM4D_PHASE_COUNTS_FROM_U16 = 0,
    EXABM4D_PHASE_ZERO_ACC_1 = 1,
    EXABM4D_PHASE_BLOCKMATCH_HT = 2,
    EXABM4D_PHASE_STAGE_HT = 3,
    EXABM4D_PHASE_NORMALIZE_BASIC = 4,
    EXABM4D_PHASE_ZERO_ACC_2 = 5,
    EXABM4D_PHASE_BLOCKMATCH_WIE = 6,
    EXABM4D_PHASE_STAGE_WIE = 7,
    EXABM4D_PHASE_NORMALIZE_OUT = 8,
    EXABM4D_PHASE_COUNT = 9
};
int exabm4d_profile_read(exabm4d_ctx* ctx, float* ms, int max_phases);

/* ---- device memory helpers (for ctypes hosts without torch) ------------------------------ */
int exabm4d_malloc(exabm4d_ctx* ctx, size_t bytes, void** dptr);
int exabm4d_free(exabm4d_ctx* ctx, void* dptr);
int exabm4d_memcpy_h2d(exabm4d_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int exabm4d_memcpy_d2h(exabm4d_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int exabm4d_memset(exabm4d_ctx* ctx, void* dst_dev, int value, size_t bytes);
/* HIP-event timing on the context's stream (bench.py measures kernels with these, not with
 * torch events, so the timing is on the stream the kernels are launched on). */
int exabm4d_event_create(exabm4d_ctx* ctx, void** ev);
int exabm4d_event_destroy(exabm4d_ctx* ctx, void* ev);
int exabm4d_event_record(exabm4d_ctx* ctx, void* ev);
int exabm4d_event_elapsed_ms(exabm4d_ctx* ctx, void* ev_start, void* ev_stop, float* ms);

/* ---- geometry + tables (host, no device) -------------------------------------------------- */
/* Reference-block grid along an axis of n voxels: 0,4,8,... plus n-8 when (n-8)%4 != 0. */
int exabm4d_grid_count(int n);
int exabm4d_grid_positions(int n, int32_t* pos);
/* The constant tables the kernels use: orthonormal DCT-II 8x8 (row u, col n) and the 8^3
 * aggregation window (z,y,x raster). Computed in double, rounded once to fp32. */
int exabm4d_tables(const exabm4d_params* p, float* dct64, float* win512);
/* Bytes of device scratch an exabm4d_denoise_*_dev call of this shape takes from the context (match table,
 * 64-bit numerator and corner-weight sums, basic estimate, work volumes, and -- since round 4 -- the 744 KB per
 * tile column of block matching's carry where the default options use it: 1.0 GB of 36.4 GB at 1024^3), under
 * the default options; the uint16 entry points add the fp32 + uint16 counts (6 bytes per voxel). */
size_t exabm4d_scratch_bytes(int nz, int ny, int nx, int batch, int stages);

/* The launch block matching chooses for a geometry (host logic only, no device call): plan = {tile slabs in z
 * (of eight cell layers, the fp32 kernel's; the integer kernel's tiles have 12 where "bm_layers" says so: fewer slabs),
 * tile rows, tile columns, slab-order parameter (0: every XCD walks its own contiguous range), carry between
 * tiles on, flat 4 x 16 tile shape}; carry_bytes = the part of the context's scratch the
 * carry takes (0 without).  Follows ctx's options "bm_carry" / "bm_xcd_mode" / "bm_layers"; ctx == NULL: the defaults. */
int exabm4d_blockmatch_plan(const exabm4d_ctx* ctx, int nz, int ny, int nx, int batch, int32_t plan[6],
                            uint64_t* carry_bytes);

/* ---- BM4D staged entry points (parity hooks; a-B1 .. a-B6 of SURVEY.md section 8) ---------- */
/* Block matching.  keys: [batch][nref][16] uint32, nref = gz*gy*gx in (z,y,x) raster of the
 * reference grid.  key = (bits(S) & 0xFFFFF800) | code, S = block SSD (fp32),
 * code = 0 for the reference block itself else 1 + ((dz+5)*11 + (dy+5))*11 + (dx+5).
 * Sorted ascending; unused slots 0xFFFFFFFF.  c_match: threshold factor (c_match*sigma^2).
 * Pointers: `vol` needs its natural (4-byte) alignment only -- the tiles are staged with 16-byte loads from
 * row starts that are dword-aligned at best whenever nx is no multiple of 4, so a view into a larger buffer is
 * the same case; `keys` must be 16-byte aligned (a reference's 16 keys are stored as four 16-byte vectors),
 * anything else is refused with EXABM4D_ERR_INVALID before a launch. */
int exabm4d_blockmatch_dev(exabm4d_ctx* ctx, const float* vol, int nz, int ny, int nx, int batch,
                           float sigma, float c_match, const exabm4d_params* p, uint32_t* keys);
/* The same on uint16 counts, the way exabm4d_denoise_u16_dev / _chunked_u16_dev match in stage 1.
 * The counts of a uint16 volume differ by exact integers whatever the offset, so block distances
 * below 2^24 are exact in fp32 and equal their integer form: where c_match * sigma^2 * 512 < 2^24
 * and nx is even the tiles run in integer arithmetic (v_pk_sub_i16 + v_dot2_i32_i16, half the
 * vector-ALU cycles); the tables are bit-identical to exabm4d_blockmatch_dev on (float)vol.
 * Option "bm_int" = 0 forces the float kernels (the parity tests compare both).
 * Pointers: `vol` needs its natural (2-byte) alignment only (it is read once, by the exabm4d_counts_from_u16_dev
 * stream, into the library's own buffers); `keys` as for exabm4d_blockmatch_dev. */
int exabm4d_blockmatch_u16_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int batch,
                               float sigma, float c_match, const exabm4d_params* p, uint32_t* keys);
/* Host decode of one reference's 16 keys at grid position (rz,ry,rx) [voxels]:
 * idx[k] = linear voxel offset of the matched block corner, dist[k] = quantised S/512,
 * *count = number of valid entries (group size is the largest power of two <= count). */
int exabm4d_match_decode(const uint32_t* keys16, int rz, int ry, int rx, int ny, int nx,
                         int64_t* idx, float* dist, int* count);
/* Collaborative filtering + aggregation.  basic == NULL: hard-threshold stage on `noisy`;
 * basic != NULL: Wiener stage (groups of `noisy` and `basic` at the same positions).
 * The sums over blocks are 64-bit integers, so the result does not depend on the order
 * the GPU adds in: num[batch][nz][ny][nx] = fl32(NUM 2^(E - 43)) with NUM = sum of
 * rint(est * fl32(u win) * 2^(43 - E)), den = fl32(CW 2^-40) convolved with the separable Kaiser window,
 * CW = sum of rint(u 2^40) on block corners, u = 1 / max(N_kept, 1) resp. 1 / max(sum W^2, 1).  Both are
 * WRITTEN (round 4; rounds 1-3 added into them).  data_exp = E: EXABM4D_DATA_EXP_AUTO takes, per volume of
 * the batch, the exponent with max |noisy| < 2^E (what exabm4d_denoise_f32_* do); a caller that shards one
 * volume passes one value for all shards (the uint16 pipelines use EXABM4D_DATA_EXP_U16 = 17).
 * Pointers: natural (4-byte) alignment suffices for noisy, basic, keys, num and den -- the kernels gather through
 * dword buffer loads and write single floats; 16-byte aligned noisy and basic additionally let the Wiener stage
 * gather from an interleaved copy (option "stage_pairvol"), which gives the same bits. */
#define EXABM4D_DATA_EXP_AUTO INT32_MIN
#define EXABM4D_DATA_EXP_U16 17
int exabm4d_stage_dev(exabm4d_ctx* ctx, const float* noisy, const float* basic,
                      const uint32_t* keys, int nz, int ny, int nx, int batch, float sigma,
                      const exabm4d_params* p, int data_exp, float* num, float* den);
/* out = num/den, then clamp to [clip_lo, clip_hi] when clip_lo <= clip_hi (np.clip,
 * data_handling.py:333); pass clip_lo > clip_hi for no clamp.  Pointers need their natural alignment only.
 * A NaN quotient stays NaN without a clamp and becomes clip_lo with one (fmaxf drops the NaN). */
int exabm4d_normalize_dev(exabm4d_ctx* ctx, const float* num, const float* den, float* out,
                          size_t n, float clip_lo, float clip_hi);

/* The two ends of exabm4d_denoise_u16_dev as staged calls, for callers that run the stages
 * themselves (z-slab sharding, distributed.py): out = (float)in - offset (read_counts,
 * machine_learning/data_handling.py:337-354) ...
 * Pointer contract of the three calls below, of the exabm4d_transform_*_dev calls and of
 * exabm4d_tile_finalize_u16_dev: every pointer needs the natural alignment of its element type only, so views
 * into larger buffers (tensor slices) are fine; when ALL pointers of a call are 16-byte aligned the stream runs
 * eight voxels per lane, else one -- the results are the same bits, and nothing outside [0, n) is written.
 * NaN: the clamp is fminf(fmaxf(x, 0), 65535) and fmaxf drops a NaN, so a NaN quantises to count 0. */
int exabm4d_counts_from_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, float* out, size_t n, float offset);
/* ... and out = uint16(rint(clamp(num/den + offset, 0, 65535))) (np.clip of data_handling.py:333 and
 * the cast of IntensityTransform.inverse, transforms.py:168-171). */
int exabm4d_normalize_u16_dev(exabm4d_ctx* ctx, const float* num, const float* den, uint16_t* out,
                              size_t n, float offset);
/* What stage 2 of the uint16 pipelines matches on: the basic estimate as the counts a uint16
 * caller would see, out = (float)rint(clamp(in + offset, 0, 65535)) - offset (a NaN gives -offset); in / out may
 * alias (in == out).  For callers
 * that run the stages themselves: exabm4d_blockmatch_dev on `out`, exabm4d_stage_dev on the unrounded `in`. */
int exabm4d_round_counts_f32_dev(exabm4d_ctx* ctx, const float* in, float* out, size_t n, float offset);

/* ---- BM4D whole pipeline ------------------------------------------------------------------- */
/* stages: 1 = hard-threshold only, 2 = hard-threshold + Wiener.  in/out may alias.
 * Working range of the fp32 forms: finite data with max |v| < 2^56 per volume.  Outside it
 * (the squares of transform coefficients leave fp32; infinities; NaNs) the kernels still run and stay inside
 * their buffers, the device raises a status bit, and the next synchronising call on the context
 * (exabm4d_denoise_f32_host itself, exabm4d_sync, exabm4d_memcpy_d2h, ...) returns EXABM4D_ERR_INVALID:
 * the results since the last synchronisation are void.  The uint16 forms are always inside. */
int exabm4d_denoise_f32_dev(exabm4d_ctx* ctx, const float* in, float* out, int nz, int ny, int nx,
                            int batch, float sigma, const exabm4d_params* p, int stages,
                            float clip_lo, float clip_hi);
/* uint16 in -> (float)in - offset -> BM4D -> + offset -> clamp [0,65535] -> rint -> uint16.
 * (read_counts + bm4d + clip + the rint/uint16 cast of IntensityTransform.inverse.)  |offset| <= 65536.
 * The result is a deterministic function of the input: two calls, the chunked / streamed forms on
 * identical padded chunks and the oracle give the same uint16 values.
 * The uint16 forms (this, the chunk-local ones) match stage 2 on the basic estimate ROUNDED TO COUNTS
 * (both matching passes run in 16-bit integer arithmetic); the fp32 forms match on the estimate
 * itself.  rint(clamp(exabm4d_denoise_f32_dev(in - offset) + offset)) is therefore a different -- equally
 * good -- result than this call's on a few per cent of the voxels. */
int exabm4d_denoise_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                            int nx, int batch, float sigma, float offset, const exabm4d_params* p,
                            int stages);
/* Chunk-local mode (BASELINE.json config 4: "256^3 chunks with 8-voxel halo"): independent units,
 * like the reference's one-bm4d()-call-per-patch pool (scripts/precompute.py:215-228).  The core
 * planes [zc0, zc1) of the input buffer `in` [nz][ny][nx] are tiled by cubic chunks of `chunk`
 * voxels (ragged last chunks allowed), chunk grid origin (zc0, 0, 0).  Every chunk is read with
 * `halo` voxels on each side -- the read window is clamped to the buffer: no padding is invented
 * at the volume's faces; planes of `in` outside [zc0, zc1) are real neighbour data, e.g. a slab's
 * exchanged halo -- and denoised IN ISOLATION by the uint16 pipeline of exabm4d_denoise_u16_dev
 * (reference grid and search clamped to the padded chunk); only its core is written, to
 * out[(zc1 - zc0)][ny][nx].  Chunks of one shape are batched per pipeline run (scratch per batch
 * bounded by option "chunk_budget_mb", default 32768).  The oracle processes the identical padded
 * arrays (oracle/bm4d_oracle.py: bm4d_u16_chunked). */
int exabm4d_denoise_chunked_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                    int nx, int zc0, int zc1, int chunk, int halo, float sigma,
                                    float offset, const exabm4d_params* p, int stages);
/* Chunk-local mode on a HOST volume of any size, streamed through the device (the harness shape of
 * scripts/evaluate_bm4dnet.py:51-181 -- a whole image in, a whole image out -- at BASELINE config 4's
 * tile size, 64 GiB of uint16, which no device call above takes in one piece).  `in` and `out` are
 * host arrays [nz][ny][nx] (pageable or pinned; they may not overlap).  One LAYER of chunks at a time:
 * planes [k chunk - halo, (k + 1) chunk + halo) go up, exabm4d_denoise_chunked_u16_dev runs on them
 * on the context's stream, the cores come down; an uploader and a downloader thread inside the call
 * keep the copies of layer k + 1 and k - 1 under the kernels of layer k.  Device memory: two windows
 * of (chunk + 2 halo) planes, two results of chunk planes, plus the scratch of the device call.  The
 * result is that of exabm4d_denoise_chunked_u16_dev on the whole volume (chunks are independent).
 * Blocks until `out` is complete. */
int exabm4d_denoise_chunked_u16_host(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                     int nx, int chunk, int halo, float sigma, float offset,
                                     const exabm4d_params* p, int stages);
/* ---- BM4D under Poisson-Gaussian noise --------------------------------------------------------
 * sCMOS counts follow var = gain (mean - offset) + read_noise^2, which no single sigma describes.  These entry
 * points stabilise the counts, denoise at sigma = 1 and invert, on the device in one call:
 *   forward  D = (2 / gain) sqrt(max(gain (v - offset) + 3 gain^2 / 8 + read_noise^2, 0))       (unit noise sigma)
 *   denoise  the fp32 pipeline of exabm4d_denoise_f32_dev on D with sigma = 1, no clip (both matching passes in
 *            the float kernels, the numerator's unit per volume from the data)
 *   inverse  0 algebraic:  offset + (((max(D,0) gain / 2)^2 - 3 gain^2 / 8) - read_noise^2) / gain
 *            1 asymptotic: the same with 1 / 8 (AnscombeTransform(unbiased_inverse=True); biased at low counts)
 *            2 closed form (Makitalo & Foi's approximation of the exact unbiased inverse; the default of the
 *              Python surface): d = max(D, d0), d0 = 2 sqrt(3/8),
 *              y = d^2/4 + (sqrt(3/2)/4)/d - (11/8)/d^2 + (5 sqrt(3/2)/8)/d^3 - 1/8 - (read_noise/gain)^2,
 *              offset + gain max(y, 0)
 *            then clamp to [0, 65535], rint, uint16.
 * All of it is fp32, one rounding per operation, constants formed in double from the struct's floats and rounded
 * once; tests/pg_pyref.py fixes the order of the operations, and the result equals that composition with the
 * oracle's fp32 pipeline bit for bit.  gain > 0, read_noise >= 0, |offset| <= 65536, all finite, inverse in
 * {0, 1, 2}; anything else is EXABM4D_ERR_INVALID before a launch. */
enum { EXABM4D_PG_INVERSE_ALGEBRAIC = 0, EXABM4D_PG_INVERSE_ASYMPTOTIC = 1, EXABM4D_PG_INVERSE_CLOSED_FORM = 2 };
typedef struct exabm4d_pg_noise {
    uint32_t size;        /* = sizeof(exabm4d_pg_noise)                                     */
    float gain;           /* counts per photo-electron: slope of variance against mean     */
    float read_noise;     /* standard deviation of the signal-independent part, counts     */
    float offset;         /* pedestal, counts                                               */
    int32_t inverse;      /* EXABM4D_PG_INVERSE_*                                           */
} exabm4d_pg_noise;
/* Whole volume, or a batch of volumes back to back; in / out are device pointers and may alias.  Scratch: that of
 * exabm4d_denoise_u16_dev.  The inverse rides in the last normalisation: the estimate never exists as fp32 in
 * HBM. */
int exabm4d_denoise_pg_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny, int nx,
                               int batch, const exabm4d_pg_noise* noise, const exabm4d_params* p, int stages);
/* Chunk-local mode and its host-streamed form: the geometry of exabm4d_denoise_chunked_u16_dev / _host, every
 * padded chunk through the stabilised pipeline above in isolation. */
int exabm4d_denoise_pg_chunked_u16_dev(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                       int nx, int zc0, int zc1, int chunk, int halo,
                                       const exabm4d_pg_noise* noise, const exabm4d_params* p, int stages);
int exabm4d_denoise_pg_chunked_u16_host(exabm4d_ctx* ctx, const uint16_t* in, uint16_t* out, int nz, int ny,
                                        int nx, int chunk, int halo, const exabm4d_pg_noise* noise,
                                        const exabm4d_params* p, int stages);
/* The two streams on their own (parity hooks): out = D of n counts; out = the chosen inverse of n stabilised
 * values, quantised.  Pointer contract of exabm4d_counts_from_u16_dev (natural alignment suffices; 16-byte
 * aligned pointers run eight voxels per lane, the same bits).  A NaN inverts like D = 0: fmaxf drops it. */
int exabm4d_gat_forward_u16_dev(exabm4d_ctx* ctx, const exabm4d_pg_noise* noise, const uint16_t* in, float* out,
                                size_t n);
int exabm4d_gat_inverse_u16_dev(exabm4d_ctx* ctx, const exabm4d_pg_noise* noise, const float* in, uint16_t* out,
                                size_t n);

/* Host-pointer form of exabm4d_denoise_f32_dev (the bm4d(z, sigma) shim calls this). */
int exabm4d_denoise_f32_host(exabm4d_ctx* ctx, const float* in, float* out, int nz, int ny, int nx,
                             int batch, float sigma, const exabm4d_params* p, int stages,
                             float clip_lo, float clip_hi);
/* The same for a batch of `batch` volumes that lie anywhere in host memory: in[i] / out[i] point to volume i
 * ([nz][ny][nx] fp32; out[i] may be in[i]).  What the per-device broker calls with every worker's patch in that
 * worker's own shared-memory segment (broker.py; reference scripts/precompute.py:215-228: one bm4d(raw, sigma)
 * per 64^3 patch and worker).  Per volume the result of exabm4d_denoise_f32_host. */
int exabm4d_denoise_f32_host_v(exabm4d_ctx* ctx, const float* const* in, float* const* out, int nz, int ny,
                               int nx, int batch, float sigma, const exabm4d_params* p, int stages,
                               float clip_lo, float clip_hi);
/* ---- BM4DNet stage (reference machine_learning/unet3d.py:137-208: Conv3d -> GroupNorm(gcd(8, C)) ->
 * LeakyReLU(0.01)): GroupNorm + LeakyReLU fused, on the NDHWC layout MIOpen's fast convolutions produce and
 * consume.  x, y: fp32 [batch][spatial][channels] (a torch channels_last_3d tensor's memory; y may be x);
 * groups of channels / groups consecutive channels; gamma, beta: [channels] or NULL; statistics in fp64,
 * combined in a fixed order.  conv_bias ([channels] or NULL): the preceding convolution's bias, added on the
 * fly -- y = lrelu(GN(x + conv_bias)) -- so that it does not cost a pass of its own.
 * Runs on `hip_stream` (the framework's current stream), not on the context's.
 * Implemented for channels % 4 == 0, (channels / groups) % 4 == 0, 256 % (channels / 4) == 0 and
 * groups <= 32 (every layer of the reference's U-Net at width_multiplier 1, 2, 4); anything else returns
 * EXABM4D_ERR_UNSUPPORTED and the caller keeps the framework's own GroupNorm.  workspace: exabm4d_groupnorm_workspace_bytes() of device memory. */
size_t exabm4d_groupnorm_workspace_bytes(int batch, size_t spatial, int channels, int groups);
int exabm4d_groupnorm_lrelu_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                      size_t spatial, int channels, int groups, const float* gamma,
                                      const float* beta, float eps, float slope, void* workspace,
                                      size_t workspace_bytes, const float* conv_bias);

/* The U-Net's resampling layers on NDHWC fp32 tensors (reference unet3d.py:211-255 MaxPool3d(2), :258-342
 * Upsample(scale_factor=2, mode="trilinear", align_corners=True)): x[batch][d][h][w][channels] ->
 * y[batch][d/2][h/2][w/2][channels] (floor) resp. y[batch][2d][2h][2w][channels]; channels % 4 == 0. */
int exabm4d_maxpool2_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch, int d,
                               int h, int w, int channels);
int exabm4d_upsample2_trilinear_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                          int d, int h, int w, int channels);

/* The same three layers on fp32, fp16 or bf16 tensors, chosen by `dtype` (an exabm4d_dtype); the fp32 entries
 * above are these with EXABM4D_DTYPE_F32.  Storage is `dtype`, arithmetic is not: a thread widens four channels
 * to fp32, the GroupNorm statistics are the fp32 kernels' (pivot-shifted fp32 sums, fp64 partials, fixed-order
 * combination), gamma, beta and conv_bias stay fp32, and every output is rounded once, to nearest even, to
 * `dtype`.  The max-pool returns one of its inputs (bit for bit, a signalling NaN quieted).  Tensors must be
 * 16-byte (fp32) or 8-byte (fp16, bf16) aligned; the shape rules, the workspace and EXABM4D_ERR_UNSUPPORTED are
 * those of the fp32 entries.  An unknown dtype is EXABM4D_ERR_INVALID. */
typedef enum exabm4d_dtype {
    EXABM4D_DTYPE_F32 = 0,
    EXABM4D_DTYPE_F16 = 1,        /* IEEE binary16 (_Float16, torch.float16)                     */
    EXABM4D_DTYPE_BF16 = 2        /* bfloat16 (__hip_bfloat16, torch.bfloat16)                   */
} exabm4d_dtype;
int exabm4d_groupnorm_lrelu_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                         int batch, size_t spatial, int channels, int groups, const float* gamma,
                                         const float* beta, float eps, float slope, void* workspace,
                                         size_t workspace_bytes, const float* conv_bias);
int exabm4d_maxpool2_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y, int batch,
                                  int d, int h, int w, int channels);
int exabm4d_upsample2_trilinear_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                             int batch, int d, int h, int w, int channels);

/* ---- BM4DNet training on NDHWC (csrc/nn_grad_kernels.hip; fp32, and fp16 / bf16 through the *_dt_dev entries
 * at the end of this section): the backward halves of the three layers above
 * and the reference's loss (machine_learning/losses.py).  All run on `hip_stream`, use no atomics and combine
 * their fp64 partial sums in a fixed order, so each result is a deterministic function of its inputs.
 *
 * exabm4d_groupnorm_lrelu_ndhwc_train_dev: exabm4d_groupnorm_lrelu_ndhwc_dev without a conv_bias (the bias stays
 * with the convolution when training), which also writes mean_rstd[batch][groups][2] = {mean, 1 / sqrt(var + eps)}
 * in fp32 -- the two numbers its own apply pass used, so that the backward normalises x with the forward's bits.
 * Same shape rules and workspace; slope must be > 0 (else EXABM4D_ERR_UNSUPPORTED), because the backward reads
 * the activation's side from y.  y should not be x: the backward needs both.
 *
 * exabm4d_groupnorm_lrelu_bwd_ndhwc_dev: x (pre-norm), y (the forward's output), dy -> dx, and dgamma, dbeta
 * [channels] (each may be NULL; gamma NULL: the non-affine module).  dz = dy (y > 0 ? 1 : slope) -- zero takes
 * the slope; xh = (x - mean) rstd; dbeta = sum dz, dgamma = sum dz xh over batch and space;
 * dx = rstd (gamma dz - m1 - xh m2), m1 and m2 the means over a (sample, group) of gamma dz and gamma dz xh.
 * Two passes over (x, y, dy).  dx may be dy.  workspace: exabm4d_groupnorm_lrelu_bwd_workspace_bytes().
 *
 * exabm4d_maxpool2_bwd_ndhwc_dev: x[batch][d][h][w][channels] (the forward's input; d, h, w >= 2),
 * dy[batch][d/2][h/2][w/2][channels] -> dx like x, every element written: dy at the position torch's max_pool3d
 * selects (scan in (d, h, w) order, replace when v > max or v is NaN: the first of equal values, +0 == -0, the
 * last NaN), 0 elsewhere, the trailing plane / row / column of an odd extent included.
 *
 * exabm4d_upsample2_trilinear_bwd_ndhwc_dev: dy[batch][2d][2h][2w][channels] -> dx[batch][d][h][w][channels], the
 * transpose of exabm4d_upsample2_trilinear_ndhwc_dev with that kernel's own fp32 indices and weights.
 *
 * exabm4d_charbonnier_loss_dev: loss[0] = mean((1 + fg_weight m) sqrt((pred - target)^2 + eps^2)) over n elements
 * in storage order, written on the device (no host synchronisation); mask: n elements of mask_bytes each
 * (4: fp32, 1: uint8 / bool), or NULL for weight 1; n is a size_t and may exceed 2^32.  Each element is
 * evaluated in fp64 and the sum rounded once.  workspace: exabm4d_charbonnier_workspace_bytes().
 * exabm4d_charbonnier_loss_bwd_dev: dpred = grad_loss[0] (1 + fg_weight m) d / sqrt(d^2 + eps^2) / n, grad_loss
 * read from device memory. */
int exabm4d_groupnorm_lrelu_ndhwc_train_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, float* y, int batch,
                                            size_t spatial, int channels, int groups, const float* gamma,
                                            const float* beta, float eps, float slope, void* workspace,
                                            size_t workspace_bytes, float* mean_rstd);
size_t exabm4d_groupnorm_lrelu_bwd_workspace_bytes(int batch, size_t spatial, int channels, int groups);
int exabm4d_groupnorm_lrelu_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, const float* y,
                                          const float* dy, float* dx, int batch, size_t spatial, int channels,
                                          int groups, const float* gamma, const float* mean_rstd, float slope,
                                          float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes);
int exabm4d_maxpool2_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* x, const float* dy, float* dx,
                                   int batch, int d, int h, int w, int channels);
int exabm4d_upsample2_trilinear_bwd_ndhwc_dev(exabm4d_ctx* ctx, void* hip_stream, const float* dy, float* dx,
                                              int batch, int d, int h, int w, int channels);
size_t exabm4d_charbonnier_workspace_bytes(void);
int exabm4d_charbonnier_loss_dev(exabm4d_ctx* ctx, void* hip_stream, const float* pred, const float* target,
                                 const void* mask, int mask_bytes, size_t n, double fg_weight, double eps,
                                 void* workspace, size_t workspace_bytes, float* loss);
int exabm4d_charbonnier_loss_bwd_dev(exabm4d_ctx* ctx, void* hip_stream, const float* pred, const float* target,
                                     const void* mask, int mask_bytes, size_t n, double fg_weight, double eps,
                                     const float* grad_loss, float* dpred);
/* The training forward and the three backward passes on tensors of `dtype` (an exabm4d_dtype), for a step under
 * fp16 / bf16 autocast; the fp32 entries above are these with EXABM4D_DTYPE_F32.  x, y, dy and dx are `dtype`;
 * gamma, beta, mean_rstd, dgamma and dbeta stay fp32 and the partial sums fp64.  A thread widens its four channels
 * exactly, evaluates the fp32 kernel's expressions and rounds each output element once, to nearest even (an fp16
 * overflow gives +-inf): from half inputs dgamma and dbeta are the bits the fp32 entry gives on the widened
 * inputs, and dx is that entry's dx rounded once.  The max-pool gradient compares the widened values and places
 * dy's elements.  A non-finite dy element is not hidden: it makes every dx of its (sample, group) non-finite and
 * dgamma / dbeta of its own channel (a parameter gradient is a per-channel sum: the group's other channels keep
 * their values), and nothing else.  Tensors 16-byte (fp32) or 8-byte (fp16, bf16) aligned, workspaces 16-byte;
 * shape rules, workspace sizes and EXABM4D_ERR_UNSUPPORTED as for the fp32 entries; an unknown dtype is
 * EXABM4D_ERR_INVALID.  The loss entries stay fp32: under autocast the network's residual sum is fp32. */
int exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, void* y,
                                               int batch, size_t spatial, int channels, int groups,
                                               const float* gamma, const float* beta, float eps, float slope,
                                               void* workspace, size_t workspace_bytes, float* mean_rstd);
int exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x,
                                             const void* y, const void* dy, void* dx, int batch, size_t spatial,
                                             int channels, int groups, const float* gamma, const float* mean_rstd,
                                             float slope, float* dgamma, float* dbeta, void* workspace,
                                             size_t workspace_bytes);
int exabm4d_maxpool2_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* x, const void* dy,
                                      void* dx, int batch, int d, int h, int w, int channels);
int exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(exabm4d_ctx* ctx, void* hip_stream, int dtype, const void* dy,
                                                 void* dx, int batch, int d, int h, int w, int channels);

/* Page-lock `bytes` of caller memory at `ptr` that the host entry points will copy from / to repeatedly (the
 * broker registers every worker's shared-memory segment once): copies become DMA transfers instead of staged
 * ones.  Unregister before the memory is unmapped. */
int exabm4d_host_register(exabm4d_ctx* ctx, void* ptr, size_t bytes);
int exabm4d_host_unregister(exabm4d_ctx* ctx, void* ptr);

/* ---- multi-GPU: halo exchange over RCCL (north_star "RCCL over xGMI only for halo
 * exchange at chunk borders") ------------------------------------------------------------------------------
 * One process per GPU.  librccl.so is dlopen()ed on first use (EXABM4D_RCCL_LIB names another copy, e.g.
 * the one a PyTorch in the same process ships); a host without RCCL gets EXABM4D_ERR_UNSUPPORTED.
 * Rank 0 draws the id (ncclGetUniqueId) and the host layer hands it to the other ranks (distributed.py does it
 * over MASTER_ADDR / MASTER_PORT without torch); exabm4d_comm_create is collective over the ranks
 * (ncclCommInitRank on the context's device). */
#define EXABM4D_COMM_ID_BYTES 128
typedef struct exabm4d_comm exabm4d_comm;
int exabm4d_comm_unique_id(uint8_t id[EXABM4D_COMM_ID_BYTES]);
int exabm4d_comm_create(exabm4d_ctx* ctx, int nranks, int rank, const uint8_t id[EXABM4D_COMM_ID_BYTES],
                        exabm4d_comm** out);
int exabm4d_comm_destroy(exabm4d_comm* comm);
/* The exchange of SURVEY.md 8e on the context's stream, no host synchronisation: ncclGroupStart; send
 * `send_lo` to rank lo_peer and receive `recv_lo` from it (bytes_lo each way); the same with hi_peer;
 * ncclGroupEnd.  A peer of -1 (or 0 bytes) skips that side (the first and the last slab).  All pointers are
 * device pointers; the planes of a z-slab are contiguous, so callers pass addresses inside their slab
 * buffers.  Replaces the torch.distributed isend / irecv pairs of distributed.HaloExchange. */
int exabm4d_halo_exchange_dev(exabm4d_ctx* ctx, exabm4d_comm* comm, int lo_peer, const void* send_lo, void* recv_lo,
                              size_t bytes_lo, int hi_peer, const void* send_hi, void* recv_hi, size_t bytes_hi);

/* *value = max over the ranks of *value (ncclAllReduce of one double on the context's stream, then a
 * synchronisation): the barrier + MAX that brackets a timed region (bench.py) without torch.distributed. */
int exabm4d_comm_max_f64_host(exabm4d_ctx* ctx, exabm4d_comm* comm, double* value);

/* ---- intensity transforms (a-D, a-E) -------------------------------------------------------
 * Pointers: natural alignment suffices, 16-byte alignment of both selects the vector path (see
 * exabm4d_counts_from_u16_dev); the uint16 forward of an asinh transform on n >= 2^20 voxels goes through a
 * 65536-entry table on either path. */
int exabm4d_transform_forward_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const uint16_t* in, float* out, size_t n);
int exabm4d_transform_forward_f32_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, float* out, size_t n);
int exabm4d_transform_inverse_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, uint16_t* out, size_t n);
int exabm4d_transform_inverse_f32_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                      const float* in, float* out, size_t n);

/* ---- overlap-tile stitching around the BM4DNet stage (a-F, a-G) ----------------------------- */
/* `starts` is a HOST array [nb][3] of patch corners (z,y,x); all other pointers are device
 * pointers.  Gather nb cubic patches of edge `patch` from vol [nz][ny][nx] into
 * out[nb][patch^3]; voxels beyond the volume are zero (add_padding, inference.py:178-199). */
int exabm4d_tile_gather_dev(exabm4d_ctx* ctx, const float* vol, int nz, int ny, int nx,
                            const int32_t* starts, int nb, int patch, float* out);
/* accum_pred[s:e] += pred[trim:-trim][: e-s]; accum_wgt[s:e] += 1 with s = start+trim,
 * e = min(s + patch-2*trim, dim) per axis, patch after patch in array order so that the fp32
 * sums are bit-identical to the reference's (inference.py:89-103). */
int exabm4d_tile_accumulate_dev(exabm4d_ctx* ctx, const float* preds, const int32_t* starts,
                                int nb, int patch, int trim, float* accum_pred, float* accum_wgt,
                                int nz, int ny, int nx);
/* out = transform.inverse(accum_pred / (accum_wgt + 1e-8f)) (inference.py:113-116).  Pointers: natural alignment
 * suffices, 16-byte alignment of all three selects the vector path (see exabm4d_counts_from_u16_dev). */
int exabm4d_tile_finalize_u16_dev(exabm4d_ctx* ctx, const exabm4d_transform* t,
                                  const float* accum_pred, const float* accum_wgt, uint16_t* out,
                                  size_t n);

/* ---- the same tiling for one brick of a stored volume (inference.predict_store) ----
 * A brick's patches are a regular grid, so no list of starts is passed and no count of patches is too many: per
 * axis (z, y, x) the index of the first patch and the number of patches; patch i starts at voxel i * stride and
 * is `patch` voxels wide (stride >= 1, 1 <= patch <= 1024, first >= 0, count >= 0).  A patch's linear index is
 * raster order over the counts, z outermost. */
typedef struct exabm4d_patch_grid {
    int32_t first[3];
    int32_t count[3];
    int32_t stride;
    int32_t patch;
} exabm4d_patch_grid;
/* out[nb][patch^3] (device fp32) = patches [k0, k0 + nb) of the grid, cut from `win`: a device uint16 array
 * [win_dims_zyx] that holds the voxels from win_origin_zyx on of a volume of vol_dims_zyx voxels.  A voxel inside
 * the volume is written as transform.forward((float)count) -- the operation exabm4d_transform_forward_u16_dev
 * applies, same bits -- and a voxel beyond the volume as 0.0f: add_padding pads the transformed image
 * (inference.py:153-199), so the pad is zero, not forward(0).  One pass: no fp32 copy of the volume exists.
 * The three triples and the grid are host arrays.  Checked before anything is launched, EXABM4D_ERR_INVALID with
 * nothing written otherwise: 0 <= k0, 0 <= nb, k0 + nb <= count_z * count_y * count_x, and per axis
 * win_origin <= first * stride and min((first + count - 1) * stride + patch, vol_dim) <= win_origin + win_dim,
 * i.e. the window holds every voxel of the grid's patches that lies inside the volume.  nb == 0 does nothing. */
int exabm4d_tile_gather_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* win_origin_zyx,
                                const int32_t* win_dims_zyx, const int32_t* vol_dims_zyx,
                                const exabm4d_transform* t, const exabm4d_patch_grid* grid, long long k0, int nb,
                                float* out);
/* out (device uint16, dense [box_dims_zyx], x fastest) = the denoised counts of the box that starts at
 * box_origin_zyx of the volume, from preds[n_patches][patch^3] (device fp32, the grid's raster order; n_patches
 * must equal the product of the counts and may be 0, preds then unused).  Per voxel p: along each axis the patch
 * indices i of the grid with i * stride + trim <= p < i * stride + trim + (patch - 2 trim) -- however many the
 * overlap makes it -- visited z outermost in increasing index with s = 0.0f; s = s + pred; w = w + 1.0f, then
 * the expression of exabm4d_tile_finalize_u16_dev.  These are the fp32 operations of exabm4d_tile_accumulate_dev
 * over the same patches in raster order followed by exabm4d_tile_finalize_u16_dev, in the same order, so the
 * counts are the same bits; a voxel no core holds comes out as transform.inverse(0).
 * Checked on the host (EXABM4D_ERR_INVALID, nothing written): 0 <= trim, 2 trim < patch, the box inside the
 * volume with extents >= 1, n_patches. */
int exabm4d_tile_stitch_u16_dev(exabm4d_ctx* ctx, const float* preds, long long n_patches,
                                const exabm4d_patch_grid* grid, int trim, const int32_t* box_origin_zyx,
                                const int32_t* box_dims_zyx, const int32_t* vol_dims_zyx,
                                const exabm4d_transform* t, uint16_t* out);

/* ---- encode half of the metric (SURVEY.md section 8 "next" row f-1) ---------------------------- */
/* Per-chunk byte-plane histograms of a uint16 volume: the front end of the reference's
 * chunked compression ratio, compute_cratio(img, Blosc(zstd, SHUFFLE), patch_shape=(64,64,64))
 * (utils/img_util.py:401-441; codec evaluate.py:40).  Blosc's SHUFFLE filter regroups a chunk's
 * bytes into a low-byte plane and a high-byte plane before the entropy coder; hist receives
 * [nchunks][2][256] uint32 counts (plane 0 = low bytes), chunks in (z,y,x) raster order of
 * ceil(n/c) chunks per axis, edge chunks truncated like numpy slicing.  From these the host
 * derives a zeroth-order entropy bound of the shuffled stream (a rate proxy; the exact Blosc/zstd
 * byte counts need the third-party codec).  Pointers: vol and hist need the natural alignment of their element
 * types only (2 and 4 bytes); vol is only read, and of hist exactly the nchunks * 512 counts are written, every
 * one of them (hist need not be zeroed). */
int exabm4d_chunk_byte_histograms_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx,
                                      int cz, int cy, int cx, uint32_t* hist);

/* Transform quantiser of the encode half (BASELINE.json config 5 "3D wavelet/DCT quantise"; the
 * reference has no such step -- it hands the denoised uint16 volume to Blosc / JPEG-XL,
 * evaluate.py:40 -- so the specification is this repo's): non-overlapping 8^3
 * blocks (edge voxels replicated), orthonormal 3-D DCT with the arithmetic of the BM4D
 * transforms, idx = (int32) rintf(c / q) (clamped to +-2^30).  idx receives ceil(nz/8) *
 * ceil(ny/8) * ceil(nx/8) blocks of 512 coefficients (block raster, then (uz, uy, ux) raster).
 * The inverse dequantises, inverts, clamps to [0, 65535] and rounds half to even.  Indices are
 * bit-exact against the oracle (orc_dctq_forward).  Pointers: vol and idx need the natural alignment of their
 * element types only (2 and 4 bytes), so views at any element offset of a larger buffer work and give the same
 * values.  The forward writes every index of every block and nothing else; the inverse writes every one of the
 * nz * ny * nx voxels and nothing else -- no voxel of the blocks' overhang beyond an extent that is not a multiple
 * of 8 is stored.  The input of either is only read. */
int exabm4d_dctq_forward_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, float q,
                             int32_t* idx);
int exabm4d_dctq_inverse_dev(exabm4d_ctx* ctx, const int32_t* idx, int nz, int ny, int nx, float q,
                             uint16_t* vol);
/* Symbol histogram of n quantisation indices for an escape-coded rate estimate: bin v + 32768
 * for -32767 <= v <= 32767, bin 0 (the escape symbol) for everything else.  hist_host[65536].  idx needs
 * 4-byte alignment only; a 16-byte aligned idx is read four indices per load. */
int exabm4d_i32_symbol_histogram_dev(exabm4d_ctx* ctx, const int32_t* idx, size_t n,
                                     uint64_t* hist_host);

/* Chunk entropy coder (BASELINE.json config 5 "entropy encode").  Replaces the
 * arithmetic behind `len(codec.encode(chunk))` in compute_cratio(img, codec, patch_shape=(64,64,64))
 * (utils/img_util.py:401-441: C-order chunks, edge chunks truncated) with the codec the reference
 * builds at evaluate.py:40 / scripts/evaluate_bm4dnet.py:140 -- Blosc(zstd, SHUFFLE).  zstd is
 * third-party and absent, so the coder is this repo's; oracle/exac_codec.c states both formats and the
 * kernels' bytes are bit-identical to it:
 *   EXAC v2 (default): every element predicted from the voxel above and the voxel in the plane
 *     before, zigzag residual -> 64-symbol alphabet + raw mantissa bits, 16 static tables per chunk
 *     selected by the neighbours' residual magnitudes, 64 interleaved rANS states (the lanes of one
 *     wave).  5.0 : 1 on the denoised bench volume where byte shuffle + zstd-5 gives 3.9 : 1.
 *   EXAC v1 (exabm4d_set_option("codec_version", 1)): byte shuffle + static order-0 rANS per byte
 *     plane (round 2's format; still decoded).
 * typesize 2 = uint16 volumes, 4 = int32 quantisation indices (exabm4d_dctq_forward_dev; coded
 * without prediction), mapped to unsigned by (v << 1) ^ (v >> 31).  version = 1 | 2 selects the format per
 * CALL (round 4: two codecs of different versions may share a context from two threads); 0 = the context's
 * "codec_version" option (default 2).
 *
 * One call codes every chunk of a volume.  out (device, may be NULL: sizes only) receives the chunk
 * streams back to back, each starting at a multiple of 16 bytes (padding zeroed); out_capacity must
 * be >= exabm4d_codec_volume_bound() (which covers either format).  offsets_dev[nchunks + 1] (device;
 * may be NULL when out is NULL) receives the start of every chunk's stream and the container length;
 * sizes_dev[nchunks] (device, may be NULL) the exact stream lengths, i.e. len(codec.encode(chunk));
 * totals_host[2] (host, may be NULL; non-NULL makes the call synchronise) = { sum of the exact
 * lengths, container bytes }.  Chunks are numbered in (z, y, x) raster order.
 *
 * Pointers of the encoder.  vol needs the natural alignment of its element type only (2 or 4 bytes) and is only
 * read; streams and sizes do not depend on where it lies (EXAC v1 counts its byte histograms 16 bytes per lane
 * where a chunk of whole 64-element rows starts on a 4-byte boundary and one element per lane elsewhere: the same
 * counts).  out must be 16-byte aligned and offsets_dev is required with it; a misaligned out, an out without
 * offsets_dev or an out_capacity below the bound gives EXABM4D_ERR_INVALID before anything is launched or
 * written.  offsets_dev needs 8-byte and sizes_dev 4-byte alignment.  Of out exactly the container
 * [0, offsets_dev[nchunks]) is written -- every stream, and zeros from the end of each stream to the next
 * multiple of 16 -- whatever out held before; [offsets_dev[nchunks], out_capacity) is unspecified (a caller must
 * not rely on it being kept or cleared), and nothing outside [out, out + out_capacity) is touched.  An
 * out_capacity of exactly the bound is accepted.  Every element of offsets_dev and sizes_dev is
 * written, and nothing around them. */
size_t exabm4d_codec_chunk_bound(size_t n_elems, int typesize);
size_t exabm4d_codec_volume_bound(int typesize, int nz, int ny, int nx, int cz, int cy, int cx);
int exabm4d_codec_encode_dev(exabm4d_ctx* ctx, const void* vol, int typesize, int version, int nz, int ny, int nx,
                             int cz, int cy, int cx, uint8_t* out, size_t out_capacity,
                             uint64_t* offsets_dev, uint32_t* sizes_dev, uint64_t* totals_host);
/* Inverse: in (in_bytes bytes on the device) + offsets_dev as produced above (or assembled by a host
 * from stored streams) -> vol[nz][ny][nx] of `typesize`-byte elements; the format version is read
 * from the first chunk's header.  Synchronises.  A malformed container -- offsets that are not
 * ascending, not 2-byte aligned or beyond in_bytes, bad magic, wrong element count or chunk shape,
 * truncated tables or words, symbols outside the alphabet -- gives EXABM4D_ERR_INVALID and never
 * reads outside [in, in + in_bytes).  Pointers: in must be 16-byte aligned (EXABM4D_ERR_INVALID otherwise, before
 * anything is launched); offsets_dev needs 8-byte alignment, vol the natural alignment of its element type only.
 * in_bytes may be exactly offsets_dev[nchunks].  in and offsets_dev are only read; every one of the nz * ny * nx
 * elements of vol is written, whatever it held before, and nothing around them. */
int exabm4d_codec_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                             int typesize, int nz, int ny, int nx, int cz, int cy, int cx, void* vol);

/* Error-bounded lossy chunk codec ("denoise, then quantise, then entropy-code" as a stored
 * format).  Chunks as in exabm4d_codec_encode_dev -- (z, y, x) raster order, edge chunks truncated to their extent
 * E -- but the chunk shape (cz, cy, cx) is NOMINAL: every axis a multiple of 8 in [8, 65528], cz * cy * cx <= 2^28,
 * not clamped to the volume.  A chunk's lossy candidate at step j is the DESIGN.md 3.10 quantisation at the step
 * Q[j] = (float) 2^((j - 4) / 4), j = 0..28 (0.5 .. 64), of its blocks (global block grid, edge voxels replicated),
 * zero-filled to the nominal (cz/8)(cy/8)(cx/8) = nb blocks; err_j = max |dctq_inverse - v| over its voxels.
 * Among the steps with err_j <= max_error the largest is taken, and the chunk stores the EXAC v2 int32 stream of
 * those indices shaped (nb, 8, 64) (mode 1) when that is shorter than the EXAC v2 uint16 stream of its voxels,
 * else the latter (mode 0; a tie too).  Every decoded voxel is within max_error of the encoder's input; with
 * max_error = 0 the decode is exact.  Chunk stream: 32-byte header ('E' 'Q' 1 mode | j* (0xFF for mode 0) 0 0 0 |
 * q as float32 bits (0 for mode 0) | Ez Ey Ex Cz Cy Cx as u16 | 8 zero bytes), then the unmodified EXAC payload.
 *
 * exabm4d_dctq_ladder_errors_dev: err[nchunks][29] (device, uint32) <- err_j of every chunk; no bound involved,
 * the per-chunk rate-distortion picture.  Does not synchronise.
 * exabm4d_bounded_volume_bound: capacity `out` needs (0 for bad sizes).
 * exabm4d_bounded_encode_dev: the contract of exabm4d_codec_encode_dev -- out (device, 16-byte aligned, may be
 * NULL: sizes only), offsets_dev[nchunks + 1], sizes_dev[nchunks] (exact stream lengths, header included),
 * totals_host[2] = { sum of the exact lengths, container bytes } (non-NULL synchronises); every stream starts at a
 * multiple of 16 bytes, padding zeroed.  0 <= max_error <= 65535.
 * exabm4d_bounded_decode_dev: container (in_bytes bytes on the device, 16-byte aligned; offsets_dev[nchunks + 1],
 * every stream at a multiple of 16 bytes) -> vol[nz][ny][nx].  Mixed containers decode in a fixed number of
 * launches.  Synchronises.  A malformed container -- offsets not ascending, unaligned or beyond in_bytes, a bad
 * header (magic, version, mode, q != Q[j*], E or C not those of the chunk), an EXAC payload that does not match
 * the header's mode and shapes, or any error the EXAC decoder finds -- gives EXABM4D_ERR_INVALID and never reads
 * outside [in, in + in_bytes).  Scratch comes from the context.
 *
 * Pointers: those of the chunk coder.  vol (encoder, ladder) needs 2-byte alignment only and is only read; err needs
 * 4-byte alignment, and every one of its nchunks * 29 entries is written (it need not be zeroed).  out and in must
 * be 16-byte aligned -- their headers and payloads move 16 bytes at a time -- and a misaligned one, an out without
 * offsets_dev or an out_capacity below exabm4d_bounded_volume_bound() gives EXABM4D_ERR_INVALID before anything
 * is launched; offsets_dev needs 8-byte and sizes_dev 4-byte alignment.  Of out exactly the container
 * [0, offsets_dev[nchunks]) is written, padding included; [offsets_dev[nchunks], out_capacity) is unspecified and
 * nothing outside [out, out + out_capacity) is touched; a capacity of exactly the bound is enough.  The decoder's
 * vol needs 2-byte alignment only; every one of its nz * ny * nx voxels is written and nothing around them, in
 * and offsets_dev are only read, and in_bytes may be exactly offsets_dev[nchunks]. */
int exabm4d_dctq_ladder_errors_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int cz, int cy,
                                   int cx, uint32_t* err);
size_t exabm4d_bounded_volume_bound(int nz, int ny, int nx, int cz, int cy, int cx);
int exabm4d_bounded_encode_dev(exabm4d_ctx* ctx, const uint16_t* vol, int nz, int ny, int nx, int cz, int cy, int cx,
                               int max_error, uint8_t* out, size_t out_capacity, uint64_t* offsets_dev,
                               uint32_t* sizes_dev, uint64_t* totals_host);
int exabm4d_bounded_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                               int nz, int ny, int nx, int cz, int cy, int cx, uint16_t* vol);

/* Error-bounded lossy chunk codec with a ladder step per 8^3 block and a per-voxel bound (format
 * "EB" version 1).  Chunks, nominal chunk shape, the ladder Q[0..28] and the transform quantiser are those of the
 * bounded codec above.  The bound of voxel v is b(v) = fg_max_error where mask[v] != 0, else max_error; mask is a
 * device uint8 array of the volume's shape or NULL (b = max_error everywhere).  0 <= fg_max_error <= max_error <=
 * 65535.  A block of the chunk's nominal grid (cz/8, cy/8, cx/8), raster order, is inside when it holds a voxel of
 * the volume.  An inside block takes the largest step j whose reconstruction is within b(v) of each of its voxels
 * inside the volume and stores its indices at Q[j]; with no such step it is verbatim and stores its voxels as int32 at
 * slot (z * 8 + y) * 8 + x (edge voxels replicated); an outside block stores zeros.  Step plane: one byte per block
 * -- j, 0xFE verbatim, 0xFF outside -- zero-padded to a multiple of 16.  Chunk stream: 32-byte header ('E' 'B' 1 mode
 * | 8 zero bytes | Ez Ey Ex Cz Cy Cx as u16 | 8 zero bytes); mode 1: the padded step plane and the EXAC v2 int32
 * stream of the (nb, 8, 64) indices, stored iff that stream is strictly shorter than mode 0: the EXAC v2 uint16
 * stream of the chunk's voxels.  Every decoded voxel is within b(v) of the encoder's input; max_error = 0 is exact.
 *
 * exabm4d_block_bounded_volume_bound: capacity `out` needs (0 for bad sizes).
 * exabm4d_block_bounded_steps_dev: plane[nchunks][nb rounded up to a multiple of 16] (device, uint8) <- the step plane
 * of every chunk, padding included, whatever mode the chunk would be stored in: the per-block picture of where the
 * bound binds.  It is not part of the store's path: it exists so that tools/bounded_sweep.py can time the select
 * kernel alone, as exabm4d_dctq_ladder_errors_dev does for the per-chunk codec.  Every byte is written; does not
 * synchronise.
 * exabm4d_block_bounded_encode_dev: the contract of exabm4d_bounded_encode_dev -- out may be NULL (sizes only),
 * offsets_dev[nchunks + 1], sizes_dev[nchunks], totals_host[2] (non-NULL synchronises), every stream at a multiple of
 * 16 bytes with zeroed padding; a misaligned out, an out without offsets_dev or an out_capacity below the bound gives
 * EXABM4D_ERR_INVALID before anything is launched, and nothing outside [out, out + out_capacity) is ever written.
 * exabm4d_block_bounded_decode_dev: container -> vol[nz][ny][nx]; synchronises.  A malformed container -- offsets not
 * ascending, unaligned or beyond in_bytes, a bad header (magic, version, mode, non-zero reserved bytes, E or C not
 * those of the chunk), a plane byte that is no step / 0xFE on an inside block or not 0xFF on an outside one, non-zero
 * plane padding, an EXAC payload that does not match mode and shapes, a verbatim value outside 0..65535, or any error
 * the EXAC decoder finds -- gives EXABM4D_ERR_INVALID and never reads outside [in, in + in_bytes).
 * Pointers: as for the bounded codec; mask needs no alignment and is only read.
 *
 * exabm4d_block_bounded_steps_tab_dev, exabm4d_block_bounded_encode_tab_dev: the two entries above
 * with a bound table.  bound_table is a device array of 65536 uint16 and caps the bound by the voxel's own value:
 * b(v) = min(bound_table[vol[v]], fg_max_error where mask[v] != 0 else max_error).  Everything else -- blocks, steps,
 * modes, the stream, which the decoder reads without the table -- and every other contract of the two entries is
 * unchanged, and every decoded voxel is within this b(v) of the encoder's input; a table of zeros is exact.
 * bound_table needs 2-byte alignment (a misaligned one gives EXABM4D_ERR_INVALID before anything is launched);
 * exactly its 65536 entries are read and nothing is written through it.  NULL: the entries above, which forward
 * here with NULL. */
size_t exabm4d_block_bounded_volume_bound(int nz, int ny, int nx, int cz, int cy, int cx);
int exabm4d_block_bounded_steps_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                    int nx, int cz, int cy, int cx, int max_error, int fg_max_error, uint8_t* plane);
int exabm4d_block_bounded_encode_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                     int nx, int cz, int cy, int cx, int max_error, int fg_max_error, uint8_t* out,
                                     size_t out_capacity, uint64_t* offsets_dev, uint32_t* sizes_dev,
                                     uint64_t* totals_host);
int exabm4d_block_bounded_steps_tab_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                        int nx, int cz, int cy, int cx, int max_error, int fg_max_error,
                                        uint8_t* plane, const uint16_t* bound_table);
int exabm4d_block_bounded_encode_tab_dev(exabm4d_ctx* ctx, const uint16_t* vol, const uint8_t* mask, int nz, int ny,
                                         int nx, int cz, int cy, int cx, int max_error, int fg_max_error,
                                         uint8_t* out, size_t out_capacity, uint64_t* offsets_dev,
                                         uint32_t* sizes_dev, uint64_t* totals_host, const uint16_t* bound_table);
int exabm4d_block_bounded_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes,
                                     const uint64_t* offsets_dev, int nz, int ny, int nx, int cz, int cy, int cx,
                                     uint16_t* vol);

/* ---- background offset + quality metrics on device (SURVEY.md section 8 "next" row f-4) --------- */
/* Element types of the metric entry points. */
enum { EXABM4D_DT_U16 = 0, EXABM4D_DT_F32 = 1, EXABM4D_DT_F64 = 2 };

/* Exact histogram of a uint16 volume resident in HBM into hist_host[65536] (host memory; the
 * call synchronises the context's stream).  It carries every order statistic the reference takes
 * with numpy on the host: estimate_offset's np.percentile of the non-zero counts
 * (machine_learning/transforms.py:414-438), the offset / all-voxel offset / median / zero
 * fraction of scripts/estimate_background_offsets.py:31-67, the median, MAD and top percentile
 * of machine_learning/metrics.py:352-424. */
int exabm4d_u16_histogram_dev(exabm4d_ctx* ctx, const uint16_t* vol, size_t n, uint64_t* hist_host);

/* One 16-bit digit of the order-preserving 64-bit key of the values widened to fp64
 * (key = bits | 2^63 for non-negative values, ~bits for negative ones), or of their absolute
 * deviation |v - center| when absdev != 0: the building block of an exact radix selection for
 * data a 65536-bin histogram cannot hold -- np.percentile of float predictions and
 * np.median(|raw - median|) in machine_learning/metrics.py:375-377,413-415.  Pass `digit`
 * (0 = most significant .. 3) counts that digit of the elements whose higher digits equal
 * `prefix`.  hist_host[65536].  vol needs the natural alignment of its element type only. */
int exabm4d_key_histogram_dev(exabm4d_ctx* ctx, const void* vol, int dtype, size_t n, int absdev,
                              double center, int digit, uint64_t prefix, uint64_t* hist_host);

/* min and max of n elements -> out_host[2] (data range of ssim3D, utils/img_util.py:985-988).  A NaN among the
 * elements makes both NaN, as np.min / np.max do.  vol needs the natural alignment of its element type only. */
int exabm4d_minmax_dev(exabm4d_ctx* ctx, const void* vol, int dtype, size_t n, double* out_host);

/* Absolute-error statistics split by a foreground mask (uint8, non-zero = foreground; NULL = all
 * background): out_host[7] = { sum |pred-ref| over foreground, the same over background,
 * foreground voxels, background voxels with pred > thr, max pred, max ref, max |pred-ref| }.  Replaces the
 * numpy passes of foreground_background_mae / false_bright_rate / mip_max_error
 * (machine_learning/metrics.py:306-381) and compute_mae / compute_lmax's reductions
 * (utils/img_util.py).  Sums are fp64; integer-valued inputs give exact results.  The comparison with thr is
 * strict.  A NaN in pred (ref) makes max pred (max ref) and max |pred-ref| NaN, like np.max, and the sum of its
 * side NaN.  pred, ref and mask need the natural alignment of their element types only. */
int exabm4d_masked_error_stats_dev(exabm4d_ctx* ctx, const void* pred, int pred_dtype,
                                   const void* ref, int ref_dtype, const uint8_t* mask, size_t n,
                                   double thr, double* out_host);

/* Sum over all voxels of the SSIM map of two volumes of the same element type, cubic uniform
 * window of `window` voxels (1..32; window i - window/2 .. i + window - window/2 - 1 per axis,
 * scipy.ndimage.uniform_filter's "reflect" boundary), constants c1 = (0.01 L)^2, c2 = (0.03 L)^2
 * supplied by the caller: ssim3D of utils/img_util.py:953-1003 is *sum_host / (nz ny nx).  a and b need the
 * natural alignment of their element type only. */
int exabm4d_ssim3d_dev(exabm4d_ctx* ctx, const void* a, const void* b, int dtype, int nz, int ny,
                       int nx, int window, double c1, double c2, double* sum_host);

/* ---- scoring one volume against another brick by brick ---------------------------- */
/* The three entries below work on a box inside a window.  A window is a dense uint16 device buffer that holds
 * the part win_origin_zyx + [0, win_dims_zyx) of a volume of vol_dims_zyx voxels (z, y, x; x fastest); the box
 * box_origin_zyx + [0, box_dims_zyx), in the volume's coordinates, lies inside the window and is what is scored.
 * ref_win, test_win (and mask_win) are windows of one geometry.  The five triples are host memory.  Every entry
 * checks the geometry on the host before anything is launched -- every extent >= 1, the volume at most 2^20 per
 * axis and 2^40 voxels, the window's origin inside the volume, the box inside the window and inside the volume --
 * and returns EXABM4D_ERR_INVALID otherwise.  A window may run past the volume's upper faces (a region read's
 * padding): nothing there is ever read.  Device buffers need the natural alignment of their element type only. */
#define EXABM4D_DIFF_BINS 131071      /* bins of a signed difference table: test - ref = -65535 .. 65535 */

/* hist_dev[(test - ref) + 65535] += 1 for every voxel of the box.  hist_dev: EXABM4D_DIFF_BINS uint64 counters
 * resident on the device, which the call ADDS to, so that the calls of all bricks of a volume build one table;
 * zero_first != 0 zeroes them before this box is counted.  With mask_win (uint16, non-zero = foreground) hist_dev
 * holds two such tables, foreground then background (2 * EXABM4D_DIFF_BINS counters), and a voxel counts in the
 * one its mask names; mask_win may be NULL.  All counters are integers: the table depends neither on the launch nor
 * on how the volume was cut into boxes.  Asynchronous on the context's stream. */
int exabm4d_diff_histogram_u16_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                                   const uint16_t* mask_win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int zero_first,
                                   uint64_t* hist_dev);

/* Maximum projections of the box along z, y and x, of ref, of test and of |test - ref|, folded (max) into nine
 * planes of the WHOLE volume's extents at the box's position.  planes_dev: 3 x (ny nx + nz nx + nz ny) 32-bit words
 * resident on the device (the device has no 16-bit atomic maximum; every value is <= 65535) -- for ref, then test,
 * then |test - ref|, the planes (y, x), (z, x) and (z, y) one after another, each dense with its last axis fastest.
 * The caller zeroes them once; max does not depend on the order, so the planes are exact for any set of boxes
 * that covers the volume.  Asynchronous on the context's stream. */
int exabm4d_mip3_u16_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                         const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                         const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, uint32_t* planes_dev);

/* exabm4d_ssim3d_dev's map summed over the box only: the same window (1..32, left = window / 2), the same
 * "reflect" boundary AT THE VOLUME'S FACES ONLY, c1 and c2 from the caller, fp64.  The sample at volume index i
 * (per axis, after reflection in [0, n)) is read from the window at i - win_origin.  The entry verifies on the
 * host that every index the box's voxels read -- box_origin - window / 2 .. box_origin + box_dims - 1 + window -
 * window / 2 - 1 per axis, reflected -- lies inside the window, and that an axis shorter than `window` is in the
 * window whole; EXABM4D_ERR_INVALID otherwise, nothing launched.  For uint16 input every running sum is an exact
 * integer, so a voxel's map value does not depend on the box it was computed in: the sums of boxes that
 * partition a volume add up to exabm4d_ssim3d_dev's but for the order of the fp64 additions, and the box equal
 * to the volume gives it bit for bit.  *sum_host is host memory; the call synchronises the context's stream. */
int exabm4d_ssim3d_box_dev(exabm4d_ctx* ctx, const uint16_t* ref_win, const uint16_t* test_win,
                           const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                           const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int window, double c1,
                           double c2, double* sum_host);

/* ---- noise table: sigma and Poisson-Gaussian parameters from the data -------------- */
#define EXABM4D_NOISE_LEVELS 49       /* quarter-octave intensity levels of exabm4d_noise_table_dev */
#define EXABM4D_NOISE_BINS 4096       /* magnitude bins per level of exabm4d_noise_table_dev */

/* One pass over a volume resident in HBM, cut into 2x2x2 cells at even coordinates (an odd trailing plane,
 * row or column is ignored; every extent >= 2).  Per cell s = the sum of its voxels v[dz][dy][dx] and d = the
 * sum of (-1)^(dz+dy+dx) v (the unnormalised Haar HHH detail; Var d = 8 sigma^2 for i.i.d. noise).  The level
 * is the quarter-octave bin of the cell mean: t = (s >> 3) + 16, e = floor(log2 t), level = 4 (e - 4) +
 * ((t >> (e - 2)) & 3), 0 .. 48; the cell counts in hist_host[level][min(|d| >> shift, EXABM4D_NOISE_BINS - 1)]
 * and adds s to sum_s_host[level].  shift: 0..6.  hist_host[EXABM4D_NOISE_LEVELS][EXABM4D_NOISE_BINS],
 * sum_s_host[EXABM4D_NOISE_LEVELS] and *skipped_host are host memory; the call synchronises the context's stream.
 * dtype EXABM4D_DT_U16: integer arithmetic throughout.  dtype EXABM4D_DT_F32 (counts minus an offset): fp32 with
 * the fixed association s = ((v000+v001)+(v010+v011))+((v100+v101)+(v110+v111)), d = ((v000-v001)-(v010-v011))-
 * ((v100-v101)-(v110-v111)); a cell with a non-finite s or d is not counted and adds one to *skipped_host (always
 * 0 for uint16); otherwise s is floored and clamped to [0, 8 * 65535] and |d| is rounded half to even (|d| >= 2^24
 * goes to the last bin), so integer-valued fp32 input in the uint16 range gives the uint16 table exactly.  All
 * counters are integers: the table does not depend on the launch.  vol needs the natural alignment of its
 * element type only. */
int exabm4d_noise_table_dev(exabm4d_ctx* ctx, const void* vol, int dtype, int nz, int ny, int nx, int shift,
                            uint64_t* hist_host, uint64_t* sum_s_host, uint64_t* skipped_host);

/* ---- measuring a volume brick by brick: the counts and every shift's noise table in one pass -- */
#define EXABM4D_COUNT_BINS 65536      /* counters of a table of the uint16 counts */
#define EXABM4D_NOISE_WIDE_BINS 16384 /* wide magnitude bins per level of exabm4d_measure_box_u16_dev */

/* One pass over a box inside a window (the geometry, its checks and its limits are those of the three entries of
 * DESIGN.md 5.17 above) that ADDS to two tables resident on the device, so that the calls of all bricks of a volume
 * build the tables of the volume; zero_first != 0 zeroes both before this box is counted.  Asynchronous on the
 * context's stream.
 *
 * counts_dev: EXABM4D_COUNT_BINS uint64 counters, counts_dev[v] += 1 for every voxel of the box: what
 * exabm4d_u16_histogram_dev gives for the volume once every box of a partition has been counted.
 *
 * noise_dev: EXABM4D_NOISE_LEVELS x EXABM4D_NOISE_WIDE_BINS uint64 counters wide[level][w], then
 * sum_s[EXABM4D_NOISE_LEVELS].  The cells are exabm4d_noise_table_dev's for the whole volume -- the 2x2x2 cells at even
 * coordinates of the VOLUME whose origin is below (dim & ~1) on every axis -- with its s, d and level bit for bit; a
 * cell is counted by the box that contains its ORIGIN, so boxes may begin and end at odd coordinates and any partition
 * of the volume counts every cell once.  The far corner of such a cell may lie one voxel outside the box: the entry
 * verifies on the host that the window contains it and returns EXABM4D_ERR_INVALID, nothing launched, otherwise.
 * The wide bin of m = |d| (< 2^18): w = m for m < 4096; otherwise, with j = floor(log2 m) - 11 (1..6),
 * w = 4096 + (j - 1) 2048 + ((m >> j) - 2048).  Its lowest value is v0(w) = w for w < 4096, else (2048 + r) << j with
 * j = (w - 4096) / 2048 + 1 and r = (w - 4096) % 2048, and exabm4d_noise_table_dev's table at any shift k = 0..6 is
 * hist_k[level][min(v0(w) >> k, EXABM4D_NOISE_BINS - 1)] += wide[level][w], exactly; sum_s does not depend on k.
 *
 * With mask_win (uint16, non-zero = foreground; a window of the same geometry) both come twice, foreground then
 * background: counts_dev holds 2 x EXABM4D_COUNT_BINS counters, noise_dev two blocks of (wide, sum_s) one after the
 * other.  A voxel counts in the table its mask names; a cell is background only if all eight of its voxels are.
 * mask_win may be NULL (one table each).  All counters are integers: the tables depend neither on the launch nor on how
 * the volume was cut into boxes.  Further limits (EXABM4D_ERR_INVALID): at most 2^31 pairs of cell rows in the box, and
 * 2^32 voxels in the share of one workgroup (one per compute unit).  Device buffers need the natural alignment of
 * their element type only; rows are read with 16-byte loads where the window's pitch, its address and its x origin
 * allow. */
int exabm4d_measure_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const uint16_t* mask_win,
                                const int32_t* vol_dims_zyx, const int32_t* win_origin_zyx,
                                const int32_t* win_dims_zyx, const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                int zero_first, uint64_t* counts_dev, uint64_t* noise_dev);

/* ---- the foreground mask of a stored volume, box by box ------------------------------
 * The geometry of exabm4d_measure_box_u16_dev: win (device, uint16, dense) holds win_origin + [0, win_dims) of a
 * volume of vol_dims voxels, the box box_origin + [0, box_dims) lies inside both.  For every voxel b of the box
 *     out[b] = value  if some voxel p of the VOLUME has vol[p] >= cut and |p - b|_1 <= radius,  else 0:
 * `radius` iterations of the 6-neighbour cross with border 0 (scipy.ndimage.binary_dilation) of vol >= cut are one
 * dilation by the L1 ball, cut at the volume's faces, so the mask of a box depends only on the voxels within `radius`
 * of it along each axis, and a partition of a volume into boxes gives the whole-volume mask.  With
 * cut = floor(thr) + 1 this is make_foreground_mask's raw > thr for integer counts; cut = 65536 makes no voxel a seed.
 * The window may reach past the volume's upper faces (a reader's padding, whatever it holds): such positions are
 * never seeds, whatever cut is.  The window must hold the box grown by `radius` per axis and cut at the volume's
 * faces; that is checked on the host.
 * out_u16 (value / 0) and out_u8 (1 / 0) are dense arrays of box_dims on the device; either may be NULL, not both.
 * counts_dev: NULL, or two uint64 words on the device, to which the call ADDS the number of seeds (vol >= cut) in
 * the box and the number of mask voxels in the box, once per workgroup; zero_first zeroes them before.  Integers:
 * they depend neither on the launch nor on how a volume was cut into boxes.
 * One launch: threshold, packing by ballot into 64-bit words in LDS, every iteration on those words, expansion.
 * Checked on the host (EXABM4D_ERR_INVALID, nothing written): non-NULL ctx, win and geometry, one output at least,
 * cut 0..65536, radius 0..EXABM4D_FG_MAX_RADIUS, value 1..65535, the geometry, at most 65535 regions of
 * 32 - 2 radius rows along z and y.  Alignment: win and out_u16 2 bytes, out_u8 none, counts_dev 8 bytes; rows are
 * loaded with 16-byte loads where win_dims[2] is a multiple of 8 (at any phase of the address), and stored with
 * 16-byte (out_u8: 8-byte) stores where box_dims[2] is, out_u8 together with out_u16 only at the same phase of eight
 * elements.  Asynchronous on the context's stream. */
#define EXABM4D_FG_MAX_RADIUS 8
int exabm4d_foreground_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx, int cut, int radius,
                                   int value, uint16_t* out_u16, uint8_t* out_u8, uint64_t* counts_dev,
                                   int zero_first);

/* ---- connected components of the seeds, and their filter by size ----------------------
 * The geometry of exabm4d_foreground_box_u16_dev.  A voxel is a SEED where win >= cut and it lies inside the
 * LABELLED REGION: the box grown by min_voxels - 1 voxels per axis and cut at the volume's faces, which the window
 * must hold (checked on the host).  What the window holds elsewhere -- a reader's padding past the faces included --
 * is never a seed and connects nothing.  Seeds are connected through faces (connectivity 6) or through faces, edges
 * and corners (26).  The label of a component is 1 + the linear (z, y, x) index WITHIN THE REGION of its first voxel
 * in raster order, background 0: a pure function of the input, bit-identical between launches, like the sizes.
 * A seed is KEPT where its component in the region has >= min_voxels voxels.  For the seeds of the box that equals
 * the same test on the components of the whole volume: a smaller component lies whole inside the region, and of a
 * larger one the region holds min_voxels voxels connected to the seed.
 *   seeds_u16   NULL, or a dense uint16 array of box_dims: 1 where the voxel is a kept seed, else 0 -- the window of
 *               a following exabm4d_foreground_box_u16_dev with cut = 1 (window = this box), which dilates it
 *   labels      NULL, or uint32 per voxel of the region (region-shaped, dense)
 *   sizes       NULL, or uint32 per voxel of the region: at index label - 1 the voxels of that component, else 0
 *   counts_dev  NULL, or three uint64 words on the device to which the call ADDS, for the count box
 *               count_origin + [0, count_dims) inside the box: its seeds, its kept seeds, and the dropped components
 *               whose first voxel lies in it; zero_first zeroes them before.  A dropped component lies whole in the
 *               region, so over a partition of a volume into count boxes the three sums are the whole volume's.
 *   scratch     device memory of scratch_bytes >= exabm4d_components_scratch_bytes(win_dims, connectivity) bytes
 *               (0: bad arguments or 2^31 voxels or more), 4-byte aligned; its contents are not kept.
 * Four launches (a tile of EXABM4D_CC_TILE_Z x _Y x _X voxels by union-find in LDS; the tile faces by atomic min on
 * the parents; roots and sizes; the filter); no workgroup waits for another.
 * Checked on the host (EXABM4D_ERR_INVALID, nothing written): non-NULL ctx, win, geometry and scratch, connectivity 6
 * or 26, min_voxels >= 1, cut 0..65536, the count box inside the box, the window holding the region, fewer than 2^31
 * labelled voxels, the scratch size; alignment: win and seeds_u16 2 bytes, labels, sizes and scratch 4, counts_dev 8.
 * Asynchronous on the context's stream. */
#define EXABM4D_CC_TILE_Z 8
#define EXABM4D_CC_TILE_Y 8
#define EXABM4D_CC_TILE_X 64
size_t exabm4d_components_scratch_bytes(const int32_t* win_dims_zyx, int connectivity);
int exabm4d_component_seeds_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                    const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                    const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                    const int32_t* count_origin_zyx, const int32_t* count_dims_zyx, int cut,
                                    int min_voxels, int connectivity, uint16_t* seeds_u16, uint32_t* labels,
                                    uint32_t* sizes, void* scratch, size_t scratch_bytes, uint64_t* counts_dev,
                                    int zero_first);

/* The same for a dense array of dims_zyx resident on the device, as box = window = volume: src is uint8 (seed where
 * non-zero; cut is ignored) or, with src_u16, uint16 (seed where >= cut).  labels, sizes: as above, of dims_zyx,
 * either may be NULL; kept_u8: NULL, or 1 / 0 bytes of dims_zyx -- the sizes are the whole array's, so min_voxels is
 * any number >= 1.  counts_dev: NULL, or the three words above for the whole array, zeroed first.  Asynchronous. */
int exabm4d_label_components_dev(exabm4d_ctx* ctx, const void* src, int src_u16, const int32_t* dims_zyx, int cut,
                                 int min_voxels, int connectivity, uint32_t* labels, uint32_t* sizes,
                                 uint8_t* kept_u8, void* scratch, size_t scratch_bytes, uint64_t* counts_dev);

/* ---- the components of a whole volume from those of its bricks' windows ------------------
 * labels (device, uint32, dense) holds the labels exabm4d_component_seeds_u16_dev made of the WINDOW win_origin + [0,
 * win_dims) of a volume of vol_dims voxels (region = window: label = 1 + the window index of the component's first
 * voxel, background 0); the BRICK brick_origin + [0, brick_dims) lies inside the window, the window inside the
 * volume, and the window has fewer than 2^31 voxels (all z, y, x).  A PROVISIONAL label is such a label in volume
 * coordinates: 1 + the linear index IN THE VOLUME of the voxel at window index label - 1, a 64-bit number.
 *
 * exabm4d_segment_collect_dev writes what a merge over all bricks needs, as pairs of uint64:
 *   own         uint32 per voxel of the window, zeroed here: at index label - 1 the voxels of that component that lie
 *               INSIDE THE BRICK (what a partition of the volume into bricks may add up)
 *   halo        (volume index of the voxel, provisional label) of every seed of the window outside the brick
 *   face        the same of every seed of the brick that lies on a low face of the brick whose brick_origin on that
 *               axis is > 0 -- a voxel that the window of the brick before it on that axis holds as halo
 *   size        (provisional label, own count) of every component with an own count > 0
 *   counts_dev  three uint64 words, zeroed here: the halo, face and size records there are
 * halo_capacity and face_capacity (records) must be at least the geometric worst case -- the voxels of the window
 * outside the brick, and the voxels of the brick on such low faces -- so those two cannot overflow.  size records are
 * always all COUNTED, and stored only below size_capacity (>= 1): where counts_dev[2] > size_capacity the buffer holds
 * size_capacity of them and the caller repeats the call with a capacity of counts_dev[2].  The order of the records
 * is not determined; their sets are.  Two launches (own counts with halo and face records, one atomic add per wave and
 * record kind; then the size records); no workgroup waits for another and no loop is without a bound.
 *
 * exabm4d_segment_relabel_dev writes the dense brick out (brick_dims elements of typesize 4 or 8 bytes): for a seed
 * the value vals[k] where keys[k] is its component's provisional label, the provisional label itself where no key
 * is, and 0 for background.  keys (ascending, distinct) and vals: n_keys uint64 each on the device; n_keys == 0
 * takes NULL.  The table is searched once per component, by the component's first voxel, into final (device,
 * typesize bytes per voxel of the window, contents not kept); a second pass streams the brick, with 16-byte loads and
 * stores for the voxels at which the address allows them.  With typesize 4 the volume has at most 2^32 - 1 voxels and
 * the caller sees to it that every val fits.
 *
 * Checked on the host (EXABM4D_ERR_INVALID, nothing written): non-NULL ctx, labels, geometry, own / final, the record
 * buffers, counts_dev and out; keys and vals unless n_keys == 0; the window inside the volume with fewer than 2^31
 * voxels and the brick inside the window; the capacities; typesize, and the volume's size with typesize 4;
 * alignment: labels and own 4 bytes, the record buffers 16, counts_dev, keys and vals 8, final and out typesize.
 * Asynchronous on the context's stream. */
int exabm4d_segment_collect_dev(exabm4d_ctx* ctx, const uint32_t* labels, const int32_t* vol_dims_zyx,
                                const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                const int32_t* brick_origin_zyx, const int32_t* brick_dims_zyx, uint32_t* own,
                                uint64_t* halo, size_t halo_capacity, uint64_t* face, size_t face_capacity,
                                uint64_t* size, size_t size_capacity, uint64_t* counts_dev);
int exabm4d_segment_relabel_dev(exabm4d_ctx* ctx, const uint32_t* labels, const int32_t* vol_dims_zyx,
                                const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                const int32_t* brick_origin_zyx, const int32_t* brick_dims_zyx, const uint64_t* keys,
                                const uint64_t* vals, size_t n_keys, int typesize, void* final, void* out);

/* dst[i] = src[i] != 0 for n elements on the device: a uint16 mask window (non-zero = foreground) as the bytes a
 * mask pool of exabm4d_scatter_boxes_dev takes.  src at an even address, dst at any; 16-byte loads and 8-byte stores
 * where src is 16-byte and dst 8-byte aligned.  n == 0 succeeds without a launch.  Asynchronous. */
int exabm4d_nonzero_u8_dev(exabm4d_ctx* ctx, const uint16_t* src, size_t n, uint8_t* dst);

/* ---- one pyramid level of a box inside a window ----------------------------------------
 * win (device, uint16, dense) holds win_origin + [0, win_dims) of a SOURCE volume of vol_dims voxels; factors_zyx are
 * 1 or 2 each, one at least 2.  The LEVEL has floor(n / f) voxels per axis (edge = EXABM4D_DS_CROP) or ceil(n / f)
 * (EXABM4D_DS_PARTIAL), and its voxel (z, y, x) reduces the source voxels [z fz, min(nz, (z + 1) fz)) x ... -- 1, 2, 4
 * or 8 of them; under CROP no window is ever cut -- by
 *     EXABM4D_DS_MODE   their most frequent value; of values equally frequent the smallest
 *     EXABM4D_DS_MEAN   sum / count rounded half to even (count is a power of two: integer arithmetic, exact)
 *     EXABM4D_DS_MAX    their largest value ("any voxel set" for a mask; the mask's value survives)
 * box_origin / box_dims are in LEVEL coordinates; out_u16 is a dense array of box_dims on the device.  The window
 * must hold [box_origin f, min(vol, (box_origin + box_dims) f)) per axis.  It may reach past the volume's upper faces
 * (a reader's padding, whatever it holds): nothing there ever enters a result.  A partition of a level into boxes
 * gives the whole level.
 * Checked on the host (EXABM4D_ERR_INVALID, nothing written): non-NULL pointers, factors, method, edge, every extent
 * >= 1, at most 2^20 voxels per axis and 2^40 in all, the window begins inside the volume, the box lies inside the
 * level, the window holds its source voxels.  Alignment: win and out_u16 2 bytes.  A lane takes 8 source voxels of a
 * row: 16-byte loads where win_dims[2] is a multiple of 8 and (factor 2 along x) the box's first source voxel lies at
 * an even element of the window's allocation; 8-byte (16-byte with a factor of 1 along x) stores where box_dims[2] is
 * a multiple of 4 (8) and out_u16 is at the phase the loads fixed; element loads and stores otherwise.
 * Asynchronous on the context's stream. */
#define EXABM4D_DS_MODE 0
#define EXABM4D_DS_MEAN 1
#define EXABM4D_DS_MAX 2
#define EXABM4D_DS_CROP 0
#define EXABM4D_DS_PARTIAL 1
int exabm4d_downsample_box_u16_dev(exabm4d_ctx* ctx, const uint16_t* win, const int32_t* vol_dims_zyx,
                                   const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                   const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                   const int32_t* factors_zyx, int method, int edge, uint16_t* out_u16);

/* ---- one pyramid level of a box of labels ------------------------------------------------
 * exabm4d_downsample_box_u16_dev's contract for a window of uint32 (typesize 4) or uint64 (typesize 8) ids, which
 * compare as UNSIGNED integers; out is a dense array of box_dims of the same type.  The reduction is a mode:
 *     EXABM4D_LABEL_ZEROS_COUNT    the most frequent value of the voxels present, of values equally frequent the
 *                                  smallest: 0 is a value like any other (EXABM4D_DS_MODE on wider values)
 *     EXABM4D_LABEL_ZEROS_IGNORE   the most frequent NON-ZERO value, of equally frequent ones the smallest; 0 only
 *                                  where every voxel present is 0
 * Checked on the host as there (EXABM4D_ERR_INVALID, nothing written), and: typesize 4 or 8, zeros, win and out
 * aligned to typesize.  A lane takes 16 bytes of a row (4 or 2 source voxels): 16-byte loads where win_dims[2] is a
 * multiple of 16 / typesize and the box's first source voxel lies at a multiple of the x factor in the window's
 * allocation (counted in elements, modulo 16 / typesize); stores of 16 / fx bytes where box_dims[2] is a multiple of
 * 16 / (typesize fx) and out is at the phase the loads fixed; element loads and stores otherwise.
 * Asynchronous on the context's stream. */
#define EXABM4D_LABEL_ZEROS_COUNT 0
#define EXABM4D_LABEL_ZEROS_IGNORE 1
int exabm4d_downsample_box_labels_dev(exabm4d_ctx* ctx, const void* win, int typesize, const int32_t* vol_dims_zyx,
                                      const int32_t* win_origin_zyx, const int32_t* win_dims_zyx,
                                      const int32_t* box_origin_zyx, const int32_t* box_dims_zyx,
                                      const int32_t* factors_zyx, int edge, int zeros, void* out);

/* ---- patch-cache foreground masks and coherence gate --
 * Batches of `batch` patches of nz x ny x nx voxels, contiguous in HBM.  Every entry point
 * synchronises the context's stream; floating-point results are deterministic (fixed mappings and
 * fixed-order reductions) and independent of the batch size. */
#define EXABM4D_LABEL_SET_MAX 1024    /* distinct positive labels one patch's device hash set holds */
#define EXABM4D_SEG_STATS_K 23        /* doubles per item of exabm4d_segment_stats_dev */
#define EXABM4D_GAUSS_MAX_RADIUS 64   /* largest radius of exabm4d_gaussian_filter3d_dev */
/* Label element types (signed types: ids <= 0 are background; unsigned: 0 is). */
enum { EXABM4D_LBL_U8 = 0, EXABM4D_LBL_U32 = 1, EXABM4D_LBL_U64 = 2, EXABM4D_LBL_I32 = 3, EXABM4D_LBL_I64 = 4 };

/* make_foreground_mask of every patch (machine_learning/metrics.py:32-62): per patch, med =
 * median(raw) and mad = median(|raw - med|) + 1e-6 by an exact radix selection, thr = med +
 * k * (1.4826 * mad), every step rounded to fp32 as numpy does; mask = raw > thr, then `dilate`
 * iterations of scipy.ndimage.binary_dilation (6-neighbour cross, border 0).  NaN propagates as in
 * numpy: a patch that holds a NaN, or whose median is infinite (|raw - med| then holds one), has a
 * NaN threshold and an empty mask; other patches of the batch are not affected.  raw: dtype
 * EXABM4D_DT_U16 or EXABM4D_DT_F32; mask: batch * nz * ny * nx bytes (0 / 1) on the device;
 * thr_host: NULL or `batch` floats. */
int exabm4d_foreground_masks_dev(exabm4d_ctx* ctx, const void* raw, int dtype, int batch, int nz, int ny,
                                 int nx, float k, int dilate, uint8_t* mask, float* thr_host);

/* scipy.ndimage.binary_dilation(m, iterations) of every patch -- the dilation of
 * make_segmentation_mask and make_skeleton_mask (metrics.py:196-198, 296-302).  in and out are
 * distinct device arrays of 0 / non-0 bytes; iterations >= 0 (0 copies). */
int exabm4d_binary_dilate_dev(exabm4d_ctx* ctx, const uint8_t* in, int batch, int nz, int ny, int nx,
                              int iterations, uint8_t* out);

/* scipy.ndimage.gaussian_filter(src.astype(float64), sigma) of every patch, bit for bit
 * (metrics.py:145, 278): axes 0, 1, 2 in turn with fp64 intermediates, mode "reflect" (repeated
 * on axes shorter than the radius), per output acc = x[0] w[0], then acc += (x[-j] + x[+j]) w[j]
 * for j = radius .. 1.  weights_host[radius + 1] is the centre-and-right half of scipy's
 * normalised kernel; radius <= EXABM4D_GAUSS_MAX_RADIUS.  src: EXABM4D_DT_F32 or EXABM4D_DT_F64;
 * out: batch * nz * ny * nx doubles on the device. */
int exabm4d_gaussian_filter3d_dev(exabm4d_ctx* ctx, const void* src, int dtype, int batch, int nz, int ny,
                                  int nx, const double* weights_host, int radius, double* out);

/* The distinct positive labels of every patch and their voxel counts (np.unique(labels[labels > 0])
 * of metrics.py:280, unordered): keys_host / counts_host [batch][EXABM4D_LABEL_SET_MAX],
 * n_host[batch] the number held, status_host[batch] 1 when the patch has more distinct labels than
 * the set holds (its keys are then incomplete and the caller must count it another way). */
int exabm4d_label_set_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, int batch, int nz, int ny,
                          int nx, uint64_t* keys_host, uint32_t* counts_host, uint32_t* n_host,
                          uint32_t* status_host);

/* Segment statistics for local_autocorr / highfreq_energy_fraction (metrics.py:65-158), one item
 * per (patch item_patch_host[i], label item_key_host[i]); a voxel belongs to the segment when its
 * label equals the key; labels <= 0 never belong to a segment, and an item key of 0 is refused with
 * EXABM4D_ERR_INVALID.  Two passes, the second centred on the means
 * of the first; out_host[i * EXABM4D_SEG_STATS_K + .] = { n, mean raw, mean (raw - smooth), sum
 * (raw - mean)^2, sum (raw - smooth - mean)^2, then for axes 0, 1, 2: pairs (v, v + lag along the
 * axis) with both voxels in the segment, mean x = raw[v], mean y = raw[v + lag], Sxx, Syy, Sxy
 * centred }.  raw: EXABM4D_DT_F32 or EXABM4D_DT_F64; smooth: NULL (raw - smooth columns 0) or
 * batch * nz * ny * nx doubles; lag >= 1. */
int exabm4d_segment_stats_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, const void* raw,
                              int raw_dtype, const double* smooth, int batch, int nz, int ny, int nx, int lag,
                              const int32_t* item_patch_host, const uint64_t* item_key_host, int n_items,
                              double* out_host);

/* ---- patch samplers (data_handling.py:446-702) ---------------------------------------
 * int(make_foreground_mask(raw, k, dilate).sum()) of every patch, as sample_bright_voxel scores its candidates
 * (data_handling.py:693): counts_host[batch] uint32.  The threshold is that of exabm4d_foreground_masks_dev, its
 * NaN rule included: a patch with a NaN threshold counts 0 and does not affect the others.  For dilate 0 or 1 no
 * mask is written to memory: a voxel counts when it is above the threshold or (dilate 1) has a face neighbour
 * inside the patch that is -- one iteration of the 6-neighbour cross with border 0.  dilate >= 2 makes the first
 * dilate - 1 iterations through the mask path into the context's memory and the last one while counting.  The
 * counts are integer sums (per wave by ballot and population count, one integer add per workgroup), so they do
 * not depend on the launch shape or on the batch size.  Checked on the host: non-NULL raw and counts_host, raw
 * EXABM4D_DT_U16 or EXABM4D_DT_F32, dilate >= 0, the sizes as for the mask entries.  thr_host: NULL or `batch`
 * floats.  One synchronisation of the context's stream, at the end. */
int exabm4d_foreground_counts_dev(exabm4d_ctx* ctx, const void* raw, int dtype, int batch, int nz, int ny, int nx,
                                  float k, int dilate, uint32_t* counts_host, float* thr_host);

/* annotation_mask of a batch of boxes (data_handling.py:446-481): mask[b] (device, batch * nz * ny * nx bytes,
 * 0 / 1) = make_segmentation_mask(labels[b], seg_dilate) | make_skeleton_mask(points, starts_host[b], (nz, ny,
 * nx), skel_dilate).  labels: NULL, or `batch` label patches on the device of label_dtype EXABM4D_LBL_*; they give
 * labels > 0, dilated seg_dilate times.  points: NULL, or npoints int32 (z, y, x) voxel triples on the device (one
 * upload per brain serves every call; with npoints == 0 the pointer is not read and the contribution is empty); a
 * point sets its voxel in every box that contains it -- box b covers starts_host[b] + [0, nz) x [0, ny) x [0, nx),
 * starts_host[batch][3] a host array -- and that mask is dilated skel_dilate times.  Duplicate points, overlapping
 * boxes and boxes away from every point are fine.  Both NULL gives EXABM4D_ERR_INVALID: the reference's None is
 * the caller's case.  Checked on the host: the pointers, the label type, dilations >= 0, the sizes as for the
 * mask entries, npoints <= 2^40.  The mask is cleared and everything launched on the context's stream: the boxes'
 * origins are kept in LDS, EXABM4D_RASTER_BOXES per launch, so a larger batch takes several launches; the stores
 * are plain bytes of 1 (equal concurrent stores, no atomics), which makes the mask deterministic.  One
 * synchronisation of the context's stream, at the end; the context's memory is used for the intermediate masks. */
#define EXABM4D_RASTER_BOXES 256
int exabm4d_annotation_masks_dev(exabm4d_ctx* ctx, const void* labels, int label_dtype, int seg_dilate,
                                 const int32_t* points, size_t npoints, const int32_t* starts_host, int skel_dilate,
                                 int batch, int nz, int ny, int nx, uint8_t* mask);

/* ---- validation scoring: evaluate_example of every patch of a batch ----------------
 * The count-space metrics behind the reference's Trainer.validate (machine_learning/metrics.py:352-424) for
 * `batch` patches of n voxels, contiguous in HBM: pred, raw and target are EXABM4D_DT_U16 or EXABM4D_DT_F32
 * (each its own type), mask holds batch * n bytes (non-zero = foreground).  Every value is widened to fp64.
 * ranks_host[4], 0-based and the same for every patch: the two median ranks ((n - 1) / 2 and n / 2) and the two
 * neighbours of the percentile's virtual index; each pair ascending and below n, the median pair equal or
 * adjacent.
 * out_host[b * EXABM4D_EVAL_K + .]:
 *    0  sum |pred - raw| over the foreground        1  sum |pred - target| over the background
 *    2  foreground voxels                           3  background voxels with pred > thr
 *    4  max pred                                    5  max raw                (NaN if the image holds one)
 *    6  med = median(raw)                           7  mad = median(|raw - med|)
 *    8  thr = med + (k * 1.4826) * (mad + 1e-6), every operation rounded on its own (no fused multiply-add)
 *    9, 10  raw at the percentile ranks             11, 12  pred at the percentile ranks
 *   13, 14, 15  1.0 if pred / raw / target holds a NaN, else 0.0
 * A median of two values is (a + b) / 2 in fp64.  NaN follows numpy: a NaN in raw (or an infinite median, which
 * makes |raw - med| hold one) gives NaN med / mad / thr and a bright count of 0; the rank values of an image
 * that holds a NaN are NaN; the sums carry NaN through.  A patch does not affect its neighbours, and the row of a
 * patch does not depend on the batch it is scored in.  batch <= EXABM4D_EVAL_MAX_BATCH, n < 2^32,
 * batch * n <= 2^40.  The operands need the natural alignment of their element types only.  One
 * synchronisation of the context's stream, at the end. */
#define EXABM4D_EVAL_K 16             /* doubles per patch of exabm4d_evaluate_batch_dev */
#define EXABM4D_EVAL_MAX_BATCH 65536
enum { EXABM4D_EVAL_MED = 6, EXABM4D_EVAL_MAD = 7, EXABM4D_EVAL_THR = 8, EXABM4D_EVAL_RAW_LO = 9,
       EXABM4D_EVAL_RAW_HI = 10, EXABM4D_EVAL_PRED_LO = 11, EXABM4D_EVAL_PRED_HI = 12, EXABM4D_EVAL_PRED_NAN = 13,
       EXABM4D_EVAL_RAW_NAN = 14, EXABM4D_EVAL_TARGET_NAN = 15 };
int exabm4d_evaluate_batch_dev(exabm4d_ctx* ctx, const void* pred, int pred_dtype, const void* raw, int raw_dtype,
                               const void* target, int target_dtype, const uint8_t* mask, int batch, size_t n,
                               double k, const uint32_t* ranks_host, double* out_host);

/* ---- region reads of a chunk store: boxes gathered from decoded chunks ---------------
 * pool (device, uint16, pool_elems elements, 2-byte alignment, only read) holds decoded chunks, each described by
 * an exabm4d_box_src: where its first voxel lies in the pool, its row and plane strides (a row is contiguous in
 * x), its origin in the array and its extent.  out[n][z][y][x] (device, C order, nbox * bz * by * bx elements of
 * out_dtype: EXABM4D_DT_U16 or EXABM4D_DT_F32, natural alignment) is the voxel p = starts_host[n] + (z, y, x):
 * the first source among box_srcs_host[n][0 .. per_box) (indices into srcs_host, -1 = unused) whose box contains
 * p supplies pool[base + (pz - z0) stride_z + (py - y0) stride_y + (px - x0)], written as it is (uint16) or as
 * (float)v - offset, one IEEE subtraction (fp32); where no source contains p, `fill` is written as given (no
 * offset; for uint16 it must be an integer in 0..65535).  This is not exabm4d_tile_gather_dev, which cuts cubes
 * out of one dense fp32 volume.
 * The three tables are host arrays.  Everything is checked on the host before anything is launched -- every
 * source inside [0, pool_elems), extents >= 1, list entries in [-1, nsrc), bz, by, bx >= 1, nbox, nsrc,
 * per_box >= 0, bz * by < 2^31, nbox * bz * by * bx <= 2^40, nbox * per_box <= 2^31, pool at an even address and
 * out at a multiple of its element size, out_dtype one of the two -- and a failure gives EXABM4D_ERR_INVALID with
 * nothing written.  The
 * tables are copied into the context's memory, the kernel is launched on the context's stream, and the call does
 * not synchronise (the host tables may be released on return).  Every element of out is written exactly once
 * and nothing around it; nbox == 0 succeeds without a launch. */
typedef struct exabm4d_box_src {
    uint64_t base;                 /* element index of the source's first voxel in pool */
    uint64_t stride_y, stride_z;   /* elements; a source row is contiguous in x */
    int32_t  z0, y0, x0;           /* its origin in the array */
    int32_t  ez, ey, ex;           /* its extent, >= 1 */
} exabm4d_box_src;
int exabm4d_gather_boxes_dev(exabm4d_ctx* ctx, const uint16_t* pool, size_t pool_elems,
                             const exabm4d_box_src* srcs_host, int nsrc, const int32_t* box_srcs_host, int per_box,
                             const int32_t* starts_host, int nbox, int bz, int by, int bx, int out_dtype,
                             float offset, double fill, void* out);

/* ---- region writes of a chunk store: boxes scattered into decoded chunks -------------
 * The mirror of exabm4d_gather_boxes_dev; both sides are exabm4d_box_src records.  boxes_host[nbox] say where each
 * source box lies in src (device, src_elems elements of src_dtype, only read: base and strides in elements of src)
 * and where it belongs in the array (origin, extent).  A record describes the written part only: the core of a
 * padded window is a record whose base points inside the window and whose strides are the window's.
 * dsts_host[ndst] are regions of pool (device, pool_elems elements of pool_dtype) -- the decoded chunks of a
 * store, as the read planner lays them out -- and dst_boxes_host[d][0 .. per_dst) lists, per destination, the boxes
 * that may touch it (indices into boxes_host, -1 = unused).  For every destination d and every voxel p of its
 * extent the listed boxes are scanned from the last entry to the first, and the first box that contains p supplies
 * the value: pool[d.base + (pz - d.z0) d.stride_z + (py - d.y0) d.stride_y + (px - d.x0)] <- src[b.base + (pz -
 * b.z0) b.stride_z + (py - b.y0) b.stride_y + (px - b.x0)].  Where no listed box contains p the pool element is not
 * written.  With lists in ascending box order this is numpy's `for n: arr[box n] = v[n]`.
 * (src_dtype, pool_dtype) is one of: (EXABM4D_DT_U16, EXABM4D_DT_U16), a copy; (EXABM4D_DT_F32, EXABM4D_DT_U16),
 * uint16(rint(clamp((float)v + offset, 0, 65535))) -- one IEEE addition, ties to even, NaN gives 0: the tail of
 * exabm4d_normalize_u16_dev and the inverse of the gather's fp32 output; (EXABM4D_DT_U8, EXABM4D_DT_U8), a copy
 * (a mask pool).  offset is used by the fp32 form only.
 * The destinations must not overlap in the pool: that is the caller's contract (the store planner's chunks never
 * do) and it is not checked.  Then every pool element is written at most once, by one thread, so overlapping boxes
 * need no atomics and the result is deterministic.  src and pool must not overlap.
 * The tables are host arrays.  Everything else is checked on the host before anything is launched -- every box
 * inside [0, src_elems), every destination inside [0, pool_elems), extents >= 1, list entries in [-1, nbox), nbox,
 * ndst, per_dst >= 0, ez * ey < 2^31 per destination, ndst * per_dst <= 2^31, src and pool at multiples of their
 * element sizes, the dtype pair one of the three -- and a failure gives EXABM4D_ERR_INVALID with nothing written.
 * The tables are copied into the context's memory, the kernel is launched on the context's stream, and the call
 * does not synchronise (the host tables may be released on return); ndst == 0 or nbox == 0 succeeds without a
 * launch. */
#define EXABM4D_DT_U8 3               /* bytes: the scatter's mask form only */
int exabm4d_scatter_boxes_dev(exabm4d_ctx* ctx, const void* src, size_t src_elems, int src_dtype,
                              const exabm4d_box_src* boxes_host, int nbox, void* pool, size_t pool_elems,
                              int pool_dtype, const exabm4d_box_src* dsts_host, int ndst,
                              const int32_t* dst_boxes_host, int per_dst, float offset);

/* ---- label codec `exac-labels`: segmentation volumes coded per 8^3 block --------
 * Lossless, for unsigned labels of typesize 4 (uint32) or 8 (uint64).  The volume (nz, ny, nx) is cut into chunks
 * (cz, cy, cx), clamped to the volume and truncated at its high faces; each chunk becomes one position-independent
 * stream: a 32-byte header, one 8-byte table entry per 8^3 block, and per block an ascending palette with packed
 * indices, or the raw values (DESIGN.md 3.13 is the specification; the stream is a pure function of the chunk).
 * A chunk holds at most 2^27 voxels, a volume at most 2^40.
 *
 * exabm4d_label_encode_bound: bytes that hold the container of any volume of this geometry (every block raw, tables,
 * headers, every stream padded to 16 bytes); 0 for a bad geometry.
 *
 * exabm4d_label_encode_dev: vol (device, C order, natural alignment) -> the container `out` (device, 16-byte aligned,
 * out_capacity >= the bound; NULL: sizes only), every stream at a multiple of 16 bytes, in chunk raster order;
 * offsets_dev[nchunks + 1] (required with out) and sizes_dev[nchunks] (optional) are device arrays;
 * totals_host[2] (optional; synchronises) = {sum of stream lengths, container bytes}.  The bytes do not depend on
 * the launch geometry, and no workgroup waits for another.
 *
 * exabm4d_label_decode_dev: the container (`in`, device, 16-byte aligned, in_bytes; offsets_dev as the encoder made
 * them) -> vol.  The kernel reads nothing outside [in, in + in_bytes) and writes nothing outside vol, whatever the
 * bytes: a stream, header or table entry that does not fit its bounds decodes to zeros, a palette index >= k is
 * clamped to k - 1 before the palette is read, and either makes the call return EXABM4D_ERR_INVALID (after it has
 * synchronised).
 *
 * exabm4d_label_gather_boxes_dev: boxes straight from coded chunks, with no decoded copy.  data (device, 16-byte
 * aligned, data_bytes) holds the streams of the touched chunks; srcs_host[nsrc] say where each lies (offset a
 * multiple of 8, offset + bytes <= data_bytes), its origin in the array (a multiple of the chunk shape) and its
 * extent (the chunk truncated to the array).  Box n is the voxels starts_host[n] + [0, bz) x [0, by) x [0, bx) of
 * the array shape3_host in chunks chunk3_host; box_srcs_host[n][0 .. per_box) lists the rows of srcs_host of the
 * chunks it touches, in raster order over its chunk range (floor(max(start, 0) / c) .. floor((min(start + b, n) - 1)
 * / c) per axis); entries past that count are ignored.  out[n][z][y][x] (device, typesize elements, natural
 * alignment) is the label there, 0 outside the array.  Every table is checked on the host before anything is
 * launched (EXABM4D_ERR_INVALID, nothing written); the kernel opens every block under its stream's bounds as the
 * decoder does and the call returns EXABM4D_ERR_INVALID for a rejected entry or a clamped index.  Synchronises. */
typedef struct exabm4d_label_src {
    uint64_t offset, bytes;        /* of the chunk's stream in data */
    int32_t  z0, y0, x0;           /* its origin in the array */
    int32_t  ez, ey, ex;           /* its extent, >= 1 */
} exabm4d_label_src;
size_t exabm4d_label_encode_bound(int typesize, int nz, int ny, int nx, int cz, int cy, int cx);
int exabm4d_label_encode_dev(exabm4d_ctx* ctx, const void* vol, int typesize, int nz, int ny, int nx, int cz, int cy,
                             int cx, uint8_t* out, size_t out_capacity, uint64_t* offsets_dev, uint32_t* sizes_dev,
                             uint64_t* totals_host);
int exabm4d_label_decode_dev(exabm4d_ctx* ctx, const uint8_t* in, size_t in_bytes, const uint64_t* offsets_dev,
                             int typesize, int nz, int ny, int nx, int cz, int cy, int cx, void* vol);
int exabm4d_label_gather_boxes_dev(exabm4d_ctx* ctx, const uint8_t* data, size_t data_bytes, int typesize,
                                   const exabm4d_label_src* srcs_host, int nsrc, const int32_t* box_srcs_host,
                                   int per_box, const int32_t* starts_host, int nbox, int bz, int by, int bx,
                                   const int32_t* shape3_host, const int32_t* chunk3_host, void* out);

#ifdef __cplusplus
}
#endif
#endif /* EXABM4D_H */
