// exabm4d_kernels.h -- host-side launcher interface between exabm4d_api.hip and *_kernels.hip.
#pragma once
#include "exabm4d_common.h"

namespace exabm4d {

// Intensity-transform constants, already rounded to fp32 exactly where numpy rounds the
// reference object's Python floats (machine_learning/transforms.py).
struct TfDev {
    int kind;     // 0 asinh, 1 anscombe, 2 linear
    int wrapped;  // OffsetTransform wrapper
    float woff;   // wrapper offset
    float maxc;   // max_count
    float off, scale, norm;                           // asinh (off/norm shared with anscombe)
    float gain, c38g2, rn2, two_over_gain, cinvg2;    // anscombe
    float mn, fden, clip, range;                      // linear: mn, mx-mn+1e-8, clip, mx-mn
};

// Poisson-Gaussian stabilisation: the un-normalised generalised Anscombe transform D of a uint16
// count and its three inverses.  Every constant is computed in double from the caller's fp32 gain, read noise and
// offset and rounded once.
struct PgDev {
    int inverse;                                      // 0 algebraic (3/8), 1 asymptotic (1/8), 2 closed form
    float gain, off, c38g2, rn2, two_over_gain;       // forward; gain, off, rn2 also in the inverses
    float cg2;                                        // inverse 0 / 1: c gain^2
    float d0, s2, k1, k2, k3;                         // closed form: 2 sqrt(3/8), (read_noise / gain)^2,
                                                      // sqrt(3/2)/4, 11/8, 5 sqrt(3/2)/8
};
hipError_t launch_pg_forward_u16(const PgDev& t, const uint16_t* in, float* out, size_t n, hipStream_t s);
hipError_t launch_pg_inverse_u16(const PgDev& t, const float* in, uint16_t* out, size_t n, hipStream_t s);

hipError_t launch_normalize(const float* num, const float* den, float* out, size_t n, float lo,
                            float hi, hipStream_t s);
hipError_t launch_counts_from_u16(const uint16_t* in, float* out, size_t n, float offset,
                                  hipStream_t s, uint16_t* out16 = nullptr);
// out_u16x != NULL: counts XOR 0x8000 (integer block matching); else out_f32 = counts - offset.  DESIGN.md 3.9.
hipError_t launch_round_counts(const float* in, float* out_f32, uint16_t* out_u16x, size_t n, float offset,
                               hipStream_t s);
hipError_t launch_normalize_u16(const float* num, const float* den, uint16_t* out, size_t n,
                                float offset, hipStream_t s);
hipError_t launch_tf_forward_u16(const TfDev& t, const uint16_t* in, float* out, size_t n,
                                 hipStream_t s);
hipError_t launch_tf_forward_u16_lut(const TfDev& t, float* lut, const uint16_t* in, float* out,
                                     size_t n, hipStream_t s);
hipError_t launch_tf_forward_f32(const TfDev& t, const float* in, float* out, size_t n,
                                 hipStream_t s);
hipError_t launch_tf_inverse(const TfDev& t, const float* in, void* out, size_t n, int quant,
                             hipStream_t s);
hipError_t launch_tile_gather(const float* vol, int nz, int ny, int nx, const int* starts, int nb,
                              int patch, float* out, hipStream_t s);
hipError_t launch_tile_accumulate(const float* preds, const int* starts, int nb, int patch, int trim,
                                  float* acc, float* wgt, int nz, int ny, int nx, hipStream_t s);
hipError_t launch_tile_finalize(const TfDev& t, const float* acc, const float* wgt, uint16_t* out,
                                size_t n, hipStream_t s);
// Overlap tiling of one brick.  TileGrid: the brick's patches as a regular grid -- per axis (z, y, x)
// the first patch index and the number of patches; patch i starts at i * stride and is `patch` voxels wide.
struct Int3 {
    int v[3];
};
struct TileGrid {
    int first[3], count[3];
    int stride, patch;
};
// patches [k0, k0 + nb) of the grid (raster order) from the uint16 window `win` (origin w0, extent wd) of a volume
// of `vol` voxels -> out[nb][patch^3] = tf_forward(count), 0.0f beyond the volume; the caller has checked the window
hipError_t launch_tile_gather_u16(const uint16_t* win, const Int3& w0, const Int3& wd, const Int3& vol,
                                  const TfDev& t, const TileGrid& g, long long k0, int nb, float* out,
                                  hipStream_t s);
// preds[count_z * count_y * count_x][patch^3] -> the counts of the box [o0, o0 + oe), dense, x fastest
hipError_t launch_tile_stitch_u16(const float* preds, const TileGrid& g, int trim, const Int3& o0, const Int3& oe,
                                  const TfDev& t, uint16_t* out, hipStream_t s);
hipError_t launch_chunk_hist(const uint16_t* vol, int nz, int ny, int nx, int cz, int cy, int cx,
                             uint32_t* hist, hipStream_t s);
hipError_t launch_dctq_forward(const uint16_t* vol, int nz, int ny, int nx, const float* dct64, float q,
                               int32_t* idx, hipStream_t s);
hipError_t launch_dctq_inverse(const int32_t* idx, int nz, int ny, int nx, const float* dct64, float q,
                               uint16_t* vol, hipStream_t s);
hipError_t launch_hist_i32_clamped(const int32_t* idx, size_t n, unsigned long long* hist, hipStream_t s);
hipError_t launch_hist_u16(const uint16_t* vol, size_t n, unsigned long long* hist, hipStream_t s);
hipError_t launch_hist_key(const void* vol, int dtype, size_t n, int absdev, double center, int digit,
                           unsigned long long prefix, unsigned long long* hist, hipStream_t s);
int masked_stats_partials(size_t n);
hipError_t launch_masked_stats(const void* pred, int pred_dtype, const void* ref, int ref_dtype,
                               const uint8_t* mask, size_t n, double thr, double* partials,
                               double* out7, hipStream_t s);
hipError_t launch_minmax(const void* a, int dtype, size_t n, double* partials, double* out2,
                         hipStream_t s);
// ---- noise table (noise_kernels.hip) ----
constexpr int NOISE_LEVELS = 49;    // quarter-octave levels of the cell mean (exabm4d.h EXABM4D_NOISE_LEVELS)
constexpr int NOISE_BINS = 4096;    // bins of |d| >> shift per level (exabm4d.h EXABM4D_NOISE_BINS)
size_t noise_table_bytes();         // hist[NOISE_LEVELS][NOISE_BINS], sum_s[NOISE_LEVELS], skipped: 64-bit each
// once per device, on the current device: raises the kernels' LDS limit; *wgs = workgroups to launch (one per CU)
hipError_t noise_table_prepare(int device, int* wgs);
// dtype 0 uint16, 1 float32; (nz / 2) * (ny / 2) < 2^31; table: noise_table_bytes() on the device, zeroed here
hipError_t launch_noise_table(const void* vol, int dtype, int nz, int ny, int nx, int shift, int wgs,
                              unsigned long long* table, hipStream_t s);
int ssim3d_partials(int nz, int ny, int nx);
int ssim3d_max_window();
hipError_t launch_ssim3d(const void* a, const void* b, int dtype, int nz, int ny, int nx, int w,
                         double C1, double C2, double* partials, double* out1, hipStream_t s);
// ---- store comparison (compare_kernels.hip, the SSIM of a box in metrics_kernels.hip) ----
// A box inside a window (all z, y, x): the dense window buffer holds w0 + [0, wd) of a volume of n voxels per axis,
// the box b0 + [0, bd) lies inside it.  The host layer checks all of that before a launch.
struct BoxGeom {
    int n[3], w0[3], wd[3], b0[3], bd[3];
};
constexpr int DIFF_BINS = 131071;   // bins of a signed difference table (exabm4d.h EXABM4D_DIFF_BINS)
// hist[(test - ref) + 65535] += 1 over the box; with a mask two tables, foreground then background
hipError_t launch_diff_hist_u16(const uint16_t* ref, const uint16_t* test, const uint16_t* mask, const BoxGeom& g,
                                unsigned long long* hist, hipStream_t s);
size_t mip3_plane_words(const BoxGeom& g);     // ny nx + nz nx + nz ny: the three planes of one volume
// planes: 3 x mip3_plane_words() 32-bit words, (yx, zx, zy) of ref, of test and of |test - ref|; max is folded in
hipError_t launch_mip3_u16(const uint16_t* ref, const uint16_t* test, const BoxGeom& g, uint32_t* planes,
                           hipStream_t s);
// partials: ssim3d_partials(bd) doubles
hipError_t launch_ssim3d_box(const uint16_t* a, const uint16_t* b, const BoxGeom& g, int w, double C1,
                             double C2, double* partials, double* out1, hipStream_t s);
// ---- measuring a box (measure_kernels.hip) ----
constexpr int COUNT_BINS = 65536;        // counters of a table of the uint16 counts (exabm4d.h EXABM4D_COUNT_BINS)
constexpr int NOISE_WIDE_BINS = 16384;   // wide bins of |d| per level (exabm4d.h EXABM4D_NOISE_WIDE_BINS)
size_t measure_counts_bytes(int tables);     // tables x COUNT_BINS 64-bit counters
size_t measure_noise_bytes(int tables);      // tables x (wide[NOISE_LEVELS][NOISE_WIDE_BINS], sum_s[NOISE_LEVELS])
// once per device, on the current device: raises the kernels' LDS limit; *wgs = workgroups to launch (one per CU)
hipError_t measure_prepare(int device, int* wgs);
// How a box is walked: 16-byte loads or element loads, the first x of a lane's groups of eight, the groups per
// row, the lanes per pair of rows, the workgroups.  false: more than 2^31 pairs of cell rows, or 2^32 voxels in one
// workgroup's share (its counters are 32-bit).
struct MeasurePlan {
    int vector_ok, xs, ngx, lx_log2;
    unsigned blocks;
};
bool measure_box_plan(const uint16_t* win, const uint16_t* mask, const BoxGeom& g, int wgs, MeasurePlan& p);
// ADDS the box's voxels to counts and the cells whose origins lie in the box to noise; with a mask window two
// tables each, foreground then background.
hipError_t launch_measure_box_u16(const uint16_t* win, const uint16_t* mask, const BoxGeom& g, const MeasurePlan& p,
                                  unsigned long long* counts, unsigned long long* noise, hipStream_t s);
// ---- the foreground mask of a box (foreground_kernels.hip) ----
constexpr int FG_MAX_RADIUS = 8;         // dilation iterations one launch makes (exabm4d.h EXABM4D_FG_MAX_RADIUS)
constexpr int FG_LANES_OUT = 61;         // output vectors of eight voxels per row of a region
constexpr int FG_STRIDE_X = 8 * FG_LANES_OUT;
// How a box is cut into regions: per axis the part [r0, r1) of the volume whose voxels may be seeds (inside the
// volume, the window and box +- radius); xs, the x of region 0's first voxel; shift (0..7), the voxel of a lane at
// which an output vector begins; whether rows are loaded / stored as vectors; the regions per axis (x, y, z).
struct FgPlan {
    int r0[3], r1[3];
    int xs, shift;
    int vec_in, vec_u16, vec_u8;
    unsigned tiles[3];
};
hipError_t foreground_prepare();         // once per device, on the current device: raises the kernel's LDS limit
// false: more regions than a launch takes
bool foreground_box_plan(const uint16_t* win, const BoxGeom& g, int radius, const uint16_t* out16, const uint8_t* out8,
                         FgPlan& p);
// out16 / out8: dense box-shaped outputs, either may be NULL; counts: NULL, or {seeds in the box, mask voxels in the
// box}, ADDED to once per workgroup
hipError_t launch_foreground_box_u16(const uint16_t* win, const BoxGeom& g, const FgPlan& p, uint32_t cut, int radius,
                                     uint32_t value, uint16_t* out16, uint8_t* out8, unsigned long long* counts,
                                     hipStream_t s);
// ---- connected components of the seeds of a window (component_kernels.hip) ----
constexpr int CC_TZ = 8, CC_TY = 8, CC_TX = 64;     // a tile, labelled in LDS (exabm4d.h EXABM4D_CC_TILE_*)
// The window w0 + [0, wd), the labelled region r0 + [0, rd) (the box grown by min_voxels - 1, cut at the volume), the
// box b0 + [0, bd) the filtered seeds are written for and the sub-box c0 + [0, cd) the counters count in (all volume
// coordinates, z y x); the tiles of the region per axis; the voxels of the region (< 2^31) and of the box.
struct CcGeom {
    int w0[3], wd[3], r0[3], rd[3], b0[3], bd[3], c0[3], cd[3];
    unsigned tiles[3];
    long long voxels, box_voxels;
};
// false: 2^31 labelled voxels or more.  grow: min_voxels - 1, clamped by the caller to what an int holds
bool components_geometry(const BoxGeom& b, const int* count0, const int* countd, long long grow, CcGeom& g);
size_t components_scratch_bytes(long long voxels);   // three 256-byte aligned arrays of 32-bit words
// parent, labels, sizes: g.voxels 32-bit words each (region-shaped); out16 / out8: dense box-shaped 1 / 0, either or
// both may be NULL; counts: NULL, or {seeds, kept seeds, dropped components}, ADDED to once per workgroup
hipError_t launch_components(const void* win, bool win_u8, const CcGeom& g, uint32_t cut, uint32_t min_voxels,
                             int connectivity, uint32_t* parent, uint32_t* labels, uint32_t* sizes, uint16_t* out16,
                             uint8_t* out8, unsigned long long* counts, hipStream_t s);
// ---- the components of a volume from those of its bricks' windows (segment_kernels.hip) ----
// The volume n, the labelled window w0 + [0, wd) inside it and the brick b0 + [0, bd) inside the window (z y x); the
// voxels of the window (< 2^31) and of the brick.  The host layer checks all of that before a launch.
struct SegGeom {
    int n[3], w0[3], wd[3], b0[3], bd[3];
    long long voxels, brick_voxels;
};
long long segment_halo_records(const SegGeom& g);    // the voxels of the window outside the brick
long long segment_face_records(const SegGeom& g);    // the voxels of the brick on a low face with b0 > 0
// own: g.voxels words, zeroed by the caller; halo / face / size: pairs of 64-bit words; counts: {halo, face, size
// records}, zeroed by the caller.  size records past size_cap are counted and not stored.
hipError_t launch_segment_collect(const uint32_t* labels, const SegGeom& g, uint32_t* own, unsigned long long* halo,
                                  unsigned long long halo_cap, unsigned long long* face, unsigned long long face_cap,
                                  unsigned long long* size, unsigned long long size_cap, unsigned long long* counts,
                                  hipStream_t s);
// final: g.voxels elements of typesize (4 or 8); out: g.brick_voxels of them
hipError_t launch_segment_relabel(const uint32_t* labels, const SegGeom& g, const unsigned long long* keys,
                                  const unsigned long long* vals, unsigned long long n_keys, int typesize, void* final,
                                  void* out, hipStream_t s);
// dst[i] = src[i] != 0 (elementwise_kernels.hip): a uint16 mask window as the bytes a mask pool takes
hipError_t launch_nonzero_u8(const uint16_t* src, uint8_t* dst, size_t n, hipStream_t s);
// ---- one pyramid level of a box (downsample_kernels.hip) ----
constexpr int DS_MODE = 0, DS_MEAN = 1, DS_MAX = 2;     // exabm4d.h EXABM4D_DS_MODE / _MEAN / _MAX
constexpr int DS_CROP = 0, DS_PARTIAL = 1;              // exabm4d.h EXABM4D_DS_CROP / _PARTIAL
// Here a BoxGeom holds the SOURCE volume's n and the window w0 + [0, wd) in source coordinates, and the box b0 + [0, bd)
// in LEVEL coordinates.  How the box is walked: the factors; ox, the level x at which piece 0 of every row begins
// (<= b0[2]); the pieces (8 source voxels each) per row; whether pieces are loaded / stored as vectors; block and grid.
struct DsPlan {
    int f[3];
    int ox, pieces;
    int vec_in, vec_out;
    unsigned block[2], grid[3];
};
void downsample_box_plan(const uint16_t* win, const BoxGeom& g, const int* factors, const uint16_t* out, DsPlan& p);
// out: a dense array of g.bd
hipError_t launch_downsample_box_u16(const uint16_t* win, const BoxGeom& g, const DsPlan& p, int method, uint16_t* out,
                                     hipStream_t s);
// ---- one pyramid level of a box of labels (label_downsample_kernels.hip) ----
constexpr int LABEL_ZEROS_COUNT = 0, LABEL_ZEROS_IGNORE = 1;    // exabm4d.h EXABM4D_LABEL_ZEROS_COUNT / _IGNORE
// The same BoxGeom and DsPlan for elements of `typesize` 4 or 8 bytes; a piece is 16 bytes of a source row.
void label_downsample_box_plan(const void* win, int typesize, const BoxGeom& g, const int* factors, const void* out,
                               DsPlan& p);
hipError_t launch_downsample_box_labels(const void* win, int typesize, const BoxGeom& g, const DsPlan& p, int zeros,
                                        void* out, hipStream_t s);
// Options of block matching (per context since round 4; exabm4d_set_option "bm_xcd_mode" / "bm_carry" / "bm_carry_fault" / "bm_layers")
struct BmOpts {
    int xcd_mode = 2;       // workgroup order: 0 = contiguous per XCD, 1 = all XCDs in one z slab of tiles (raster), n >= 2 = in strips of n tile rows
    int carry = 1;          // tiles of a column hand their top cell layer upwards (0 off, 1 automatic, 2 forced)
    int carry_fault = 0;    // debug: every carry wait counts as run out (the error path's test)
    int layers = 0;         // cell layers per tile of the integer kernel: 0 automatic, 8 or 12 forced
};
// The launch block matching chooses for a geometry (bm_kernels.hip: bm_plan), evaluated once per launch
struct BmPlan {
    int tz, ty, tx;         // tile slabs, tile rows, tile columns
    int layers;             // cell layers per tile of the integer kernel (8 or 12); `tz` counts tiles of that many
    int tz_f32;             // tile slabs of the fp32 kernel, always 8 layers per tile (= tz when layers == 8)
    int xq;                 // slab-order parameter (0: every XCD walks its own contiguous range)
    int carry;              // carry between the tiles of a column on
    int flat;               // 4 x 16 tile shape instead of 8 x 8
    int strip, fault;
    size_t carry_bytes;     // device memory the launch needs for the carry (slots + done[] + ticket), 0 without
};
BmPlan bm_plan(const VolGeom& g, int batch, const BmOpts& opt);
hipError_t launch_blockmatch(const float* vol, const VolGeom& g, int batch, uint32_t keymax,
                             uint32_t* keys, hipStream_t stream, int force_generic, int guarded,
                             const uint16_t* vol16, const BmPlan& plan, void* carry_mem, unsigned* status);
// Options of the stage kernels (per context since round 4; exabm4d_set_option "stage_pairvol" / "stage_strip" /
// "stage_chunks"): Wiener gathers from an interleaved (noisy, basic) volume; tile columns walked in strips of n
// tile rows (0 = raster); diagnostic override of the z chunk count (0 = automatic).
struct StageOpts {
    int pairvol = 1;
    int strip = 3;
    int chunks = 0;
};
// One stage: adds to num (int64 fixed point) and to the corner weights cw; see stage_kernels.hip.
hipError_t launch_stage(const float* noisy, const float* basic, const uint32_t* keys,
                        const VolGeom& g, int batch, const float* dct64, const float* win_dev,
                        float thr, float sigma2, const double* qscale, long long* num,
                        unsigned long long* cw, hipStream_t stream, const StageOpts& opt,
                        float* pair = nullptr, int pair_ready = 0);
// The numerator's unit per volume: qscale[2 b] = 2^(43 - E), qscale[2 b + 1] = 2^(E - 43).
// fixed_exp != INT32_MIN: E = fixed_exp for every volume (the uint16 entry points: 17); else E from the
// largest |v| bit pattern of volume b of `vol` (maxbits: `batch` words of scratch).  No host synchronisation.
hipError_t launch_qscale(const float* vol, size_t nvox, int batch, int fixed_exp, unsigned* maxbits,
                         double* qscale, hipStream_t s, unsigned* status = nullptr);
// den = fl32(cw 2^-40) (*) win for the separable window win = k (x) k (x) k: fused x / y pass cw -> tmp,
// z pass tmp -> den (written).
hipError_t launch_den_from_corners(const unsigned long long* cw, float* tmp, float* den, int nz, int ny, int nx,
                                   int batch, const float* win1d, hipStream_t s);
// The pipelines' form: only the x / y passes (cw -> tmp); the z pass rides with the normalisation:
// out = fl32(fl64(num) 2^(E - 43)) / (tmp (*)_z win), then clip (f32) or + offset, clamp, rint (uint16).
hipError_t launch_den_xy_from_corners(const unsigned long long* cw, float* tmp, int nz, int ny, int nx, int batch,
                                      const float* win1d, hipStream_t s);
// What the fused normalisation -- and so a whole pipeline run -- writes, exactly one of: fp32, optionally clamped
// to [lo, hi]; uint16 = quantise(estimate + offset); uint16 = quantise(pg inverse(estimate)).
struct NormOut {
    float* f32; bool clip; float lo, hi;
    uint16_t* u16; float offset; const PgDev* pg;
    static NormOut to_f32(float* out) { return {out, false, 0.0f, 0.0f, nullptr, 0.0f, nullptr}; }
    // the C ABI's convention, translated here and nowhere else: clip_lo > clip_hi means "no clip"
    static NormOut to_f32_abi_clip(float* out, float clip_lo, float clip_hi) {
        return {out, clip_lo <= clip_hi, clip_lo, clip_hi, nullptr, 0.0f, nullptr};
    }
    static NormOut to_u16(uint16_t* out, float offset) { return {nullptr, false, 0.0f, 0.0f, out, offset, nullptr}; }
    static NormOut to_u16_pg(uint16_t* out, const PgDev* pg) { return {nullptr, false, 0.0f, 0.0f, out, 0.0f, pg}; }
};
// The sums a normalisation reads: the int64 numerator, its units, the denominator after its x / y passes.
struct NormSums {
    const long long* num; const double* qscale; const float* txy;
    int nz, ny, nx, batch;
    const float* win1d;
};
// Optional by-products of an fp32 normalisation, each written only where the launch can (NormWrote says which).
// pair: the interleaved (pair_src, out) volume of the Wiener stage's gathers; wide form, 16-byte aligned.
// round16: the UNCLIPPED estimate rounded to counts XOR 0x8000, rint(clamp(out + round_offset, 0, 65535)), what
// stage 2 of the uint16 pipelines matches on; 8-byte aligned.
struct NormSide { const float* pair_src; float* pair_out; uint16_t* round16; float round_offset; };
struct NormWrote { hipError_t err; bool pair, round16; };
NormWrote launch_normalize_zconv(const NormSums& in, const NormOut& out, hipStream_t s, const NormSide* side = nullptr);
// BM4DNet stage: GroupNorm + LeakyReLU on an NDHWC tensor x[batch][spatial][C] (nn_kernels.hip); y may be x.
// Requires C % 4 == 0, (C / G) % 4 == 0, 256 % (C / 4) == 0, G <= 32.  T: float, _Float16 or __bf16 (the
// storage of torch.bfloat16); gamma, beta, cbias and the workspace's statistics are fp32 / fp64 for all three.
size_t groupnorm_workspace_bytes(int batch, size_t spatial, int C, int G);
template <typename T>
hipError_t launch_groupnorm_lrelu_ndhwc(const T* x, T* y, int batch, size_t spatial, int C, int G,
                                        const float* gamma, const float* beta, float eps, float slope,
                                        void* workspace, hipStream_t s, const float* cbias = nullptr,
                                        float* stats = nullptr);
// MaxPool3d(2) (floor) and trilinear x2 up-sampling (align_corners) on NDHWC tensors of T (as above), C % 4 == 0
template <typename T>
hipError_t launch_maxpool2_ndhwc(const T* x, T* y, int batch, int D, int H, int W, int C, hipStream_t s);
template <typename T>
hipError_t launch_upsample2_trilinear_ndhwc(const T* x, T* y, int batch, int D, int H, int W, int C, hipStream_t s);
// Backward passes of the three layers above, on tensors of T as above (x, y, dy, dx in T; gamma, stats, dgamma,
// dbeta fp32; the arithmetic is the fp32 instance's, each dx element rounded once), and the training loss, fp32
// (nn_grad_kernels.hip).  stats: the [batch][G][2] = {mean, rstd} that launch_groupnorm_lrelu_ndhwc wrote; y: that
// forward's output; gamma, dgamma, dbeta may be NULL; slope > 0.  The resampling gradients take the FORWARD
// INPUT's extents D, H, W (max-pool: all >= 2); the max-pool's dx, [batch][D][H][W][C], is written completely.
size_t groupnorm_bwd_workspace_bytes(int batch, size_t spatial, int C, int G);
template <typename T>
hipError_t launch_groupnorm_lrelu_bwd_ndhwc(const T* x, const T* y, const T* dy, T* dx, int batch, size_t spatial,
                                            int C, int G, const float* gamma, const float* stats, float slope,
                                            float* dgamma, float* dbeta, void* workspace, hipStream_t s);
template <typename T>
hipError_t launch_maxpool2_bwd_ndhwc(const T* x, const T* dy, T* dx, int batch, int D, int H, int W, int C,
                                     hipStream_t s);
template <typename T>
hipError_t launch_upsample2_trilinear_bwd_ndhwc(const T* dy, T* dx, int batch, int D, int H, int W, int C,
                                                hipStream_t s);
// mean((1 + w m) sqrt((pred - target)^2 + eps^2)) over n elements -> loss[0], and its gradient times grad_loss[0];
// mask: NULL, or n elements of mask_bytes (4: float, 1: uint8 / bool) each
size_t charbonnier_workspace_bytes();
hipError_t launch_charbonnier_loss(const float* pred, const float* target, const void* mask, int mask_bytes,
                                   size_t n, double w, double eps, void* workspace, float* loss, hipStream_t s);
hipError_t launch_charbonnier_loss_bwd(const float* pred, const float* target, const void* mask, int mask_bytes,
                                       size_t n, double w, double eps, const float* grad_loss, float* dpred,
                                       hipStream_t s);
// staged entry point: num_f = fl32(fl64(num) 2^(E - 43))
hipError_t launch_num_to_float(const long long* num, const double* qscale, float* out, size_t nvox, int batch,
                               hipStream_t s);

// ---- chunk-local mode (elementwise_kernels.hip) ------------------------------------------------------
// One batch of equally shaped padded chunks out of a sub-grid of chunks (sgz x sgy x sgx chunks
// whose first core starts at (z0, y0, x0)); chunk number first + b of the sub-grid is batch entry b.
struct ChunkBatch {
    int nz, ny, nx;          // input buffer
    int z0, y0, x0;          // core origin of sub-grid chunk (0, 0, 0)
    int cz, cy, cx;          // core pitch of the chunk grid
    int ez, ey, ex;          // core extent of the chunks of this sub-grid (<= pitch)
    int pz, py, px;          // padded extent = halo in front (cut at the buffer) + core + halo behind
    int lz, ly, lx;          // voxels in front of the core inside the padded chunk
    int sgy, sgx;            // sub-grid chunks along y, x
    int first, count;        // batch = sub-grid chunks [first, first + count)
    int out_z0;              // output plane 0 is input plane out_z0
};
// What a chunk's voxels are on the fp32 side: counts - offset (pg == NULL), or the stabilised D.
// gather: u16 -> fp32 padded chunks (out16, offset form only: also the counts XOR 0x8000); scatter: the cores back,
// + offset or the pg inverse, clamp, rint, u16.
struct ChunkMap { float offset; const PgDev* pg; };
hipError_t launch_chunk_gather(const uint16_t* in, const ChunkBatch& cb, const ChunkMap& m, float* out,
                               hipStream_t s, uint16_t* out16 = nullptr);
hipError_t launch_chunk_scatter(const float* est, const ChunkBatch& cb, const ChunkMap& m, uint16_t* out,
                                hipStream_t s);

// ---- chunk entropy coder (rans_kernels.hip) ----------------------------------------
struct CodecGeom {
    int ts;                  // element bytes: 2 (uint16) or 4 (int32, zigzag mapped)
    int nz, ny, nx;          // volume, elements
    int cz, cy, cx;          // chunk shape (clamped to the volume)
    int gz, gy, gx;          // chunks per axis
    int nchunks;
    size_t slot_hdr;         // scratch slot of one chunk: header + tables ...
    size_t slot_plane;       // ... then `ts` stream regions of this many bytes
    size_t slot_bytes;
    size_t chunk_elems;      // cz * cy * cx: stride of a chunk in the v2 encoder's code scratch
    int version;             // stream format: 1 = byte planes, 2 = predictive context model (3.11b)
};
int make_codec_geom(int ts, int nz, int ny, int nx, int cz, int cy, int cx, CodecGeom& g, int version = 2);
size_t codec_chunk_bound(size_t n, int ts);
size_t codec_volume_bound(const CodecGeom& g);
void codec_fill_rcp_table(uint32_t* tab /* [4097][2]: reciprocal, shift */);
// sizes[nchunks], offsets[nchunks + 1], totals[2] are device arrays; out == nullptr skips the packing
// slots: nchunks * g.slot_bytes of scratch, followed (v2) by codec2_work_bytes(g) more
hipError_t launch_rans_encode(const void* vol, const CodecGeom& g, const uint32_t* rcp_tab, uint8_t* slots,
                              uint32_t* sizes, unsigned long long* offsets, unsigned long long* totals,
                              uint8_t* out, hipStream_t s);
hipError_t launch_rans_decode(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                              const CodecGeom& g, void* vol, uint32_t* status, hipStream_t s);
// EXAC v2 (rans2_kernels.hip); stage 0: code every chunk into its slot, stage 1: pack the slots
size_t codec2_chunk_bound(size_t n, int ts);
void codec2_slot_layout(size_t chunk_elems, int ts, size_t& slot_hdr, size_t& slot_bytes);
size_t codec2_work_bytes(const CodecGeom& g);      // encoder scratch behind the slots: codes + histograms
hipError_t launch_rans2_encode(const void* vol, const CodecGeom& g, const uint32_t* rcp_tab, uint8_t* slots,
                               uint8_t* work, uint32_t* sizes, uint8_t* out, const unsigned long long* offsets,
                               int stage, hipStream_t s);
hipError_t launch_rans2_decode(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                               const CodecGeom& g, void* vol, uint32_t* status, hipStream_t s);
// The same decoder over a device-side list of chunks: workgroup k (< grid, which must be >= *count) decodes chunk
// chunk[k] of g from bytes [range[2k], range[2k + 1]) of `in`; workgroups k >= *count return at once.
struct DecodeList {
    const uint32_t* chunk;
    const unsigned long long* range;
    const uint32_t* count;
};
hipError_t launch_rans2_decode_list(const uint8_t* in, size_t in_bytes, const DecodeList& lst, unsigned grid,
                                    const CodecGeom& g, void* vol, uint32_t* status, hipStream_t s);
// offsets[c] = sum of the 16-byte-aligned sizes before c, offsets[n] and totals = {sum of sizes, container bytes}
hipError_t launch_codec_scan(const uint32_t* sizes, int nchunks, unsigned long long* offsets,
                             unsigned long long* totals, hipStream_t s);

// ---- error-bounded lossy chunk codec (bounded_kernels.hip) ---------------------------------
constexpr int BQ_STEPS = 29;        // the step ladder Q[j] = 2^((j - 4) / 4), j = 0..28 (host table)
constexpr int BQ_HEADER = 32;       // bytes of a chunk stream's header in front of its EXAC payload
struct BoundedGeom {
    int nz, ny, nx;          // volume
    int cz, cy, cx;          // nominal chunk shape, every axis a multiple of 8 (not clamped to the volume)
    int gz, gy, gx;          // chunks per axis
    int nchunks;
    int cbz, cby, cbx;       // 8^3 blocks per chunk axis (nominal)
    int nb;                  // blocks per chunk: the index chunk is (nb, 8, 64) int32
};
int make_bounded_geom(int nz, int ny, int nx, int cz, int cy, int cx, BoundedGeom& g);
// err[nchunks][BQ_STEPS] (zeroed by the caller) <- max over the chunk's voxels of |dctq round trip at Q[j] - v|
hipError_t launch_bq_ladder(const uint16_t* vol, const BoundedGeom& g, const float* dct64, const float* qtab,
                            uint32_t* err, hipStream_t s);
// jsel[c] = max{j : err[c][j] <= delta} or -1, qsel[c] = Q[jsel] or 0
hipError_t launch_bq_select(const uint32_t* err, int nchunks, uint32_t delta, const float* qtab, int32_t* jsel,
                            float* qsel, hipStream_t s);
// chunk-major indices at q = qsel[c]: idx[c][nb][512]; blocks outside the volume and chunks with qsel 0 are zero
hipError_t launch_bq_forward(const uint16_t* vol, const BoundedGeom& g, const float* dct64, const float* qsel,
                             int32_t* idx, hipStream_t s);
// mode per chunk from the two candidates' exact sizes, stream sizes = header + payload, offsets by scan, then
// (out != NULL) headers + the chosen payloads
hipError_t launch_bq_assemble(const BoundedGeom& g, const int32_t* jsel, const float* qsel,
                              const uint8_t* lossy, const unsigned long long* lossy_off, const uint32_t* lossy_sz,
                              const uint8_t* lossless, const unsigned long long* lossless_off,
                              const uint32_t* lossless_sz, uint32_t* sizes, unsigned long long* offsets,
                              unsigned long long* totals, uint8_t* out, hipStream_t s);
// decode, step 1: validate every chunk's offsets and header, record mode / q, and list the chunks of either mode
// (lists: chunk[2][nchunks], range[2][2 nchunks], count[2], zeroed by the caller); status |= 32 / 64 on a bad
// header / offsets
hipError_t launch_bq_parse(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                           const BoundedGeom& g, const float* qtab, uint32_t* mode, float* qv, uint32_t* lchunk,
                           unsigned long long* lrange, uint32_t* lcount, uint32_t* status, hipStream_t s);
// decode, last step: inverse DCT of the mode-1 chunks' indices at their own q into the volume
hipError_t launch_bq_inverse(const int32_t* idx, const BoundedGeom& g, const float* dct64, const uint32_t* mode,
                             const float* qv, uint16_t* vol, hipStream_t s);

// ---- error-bounded codec, a step per 8^3 block (block_bounded_kernels.hip) ------------------
// Geometry, ladder and header length are the bounded codec's.  A chunk's step plane: one byte per block of the
// nominal grid in raster order (step, 0xFE verbatim, 0xFF outside the volume), zero-padded to bb_plane_bytes().
uint32_t bb_plane_bytes(const BoundedGeom& g);
// plane[c][block] (padding zeroed by the caller) and the chunk-major indices idx[c][nb][512] in one pass: per inside
// block the largest step whose reconstruction is within delta (delta_fg where mask != 0; mask may be NULL) of every
// voxel of the block inside the volume, its indices at that step; its voxels if there is no such step; zeros outside.
// table: NULL, or 65536 uint16 on the device; the bound of a voxel of value V is then further capped by table[V]
// 
hipError_t launch_bb_select(const uint16_t* vol, const uint8_t* mask, const uint16_t* table, const BoundedGeom& g,
                            const float* dct64, const float* qtab, uint32_t delta, uint32_t delta_fg, uint8_t* plane,
                            int32_t* idx, hipStream_t s);
// launch_bq_assemble with the plane in front of a mode-1 payload (plane: 16-byte aligned)
hipError_t launch_bb_assemble(const BoundedGeom& g, const uint8_t* plane, const uint8_t* lossy,
                              const unsigned long long* lossy_off, const uint32_t* lossy_sz, const uint8_t* lossless,
                              const unsigned long long* lossless_off, const uint32_t* lossless_sz, uint32_t* sizes,
                              unsigned long long* offsets, unsigned long long* totals, uint8_t* out, hipStream_t s);
// launch_bq_parse for this format: offsets, header and step plane of every chunk; status |= 32 / 64
hipError_t launch_bb_parse(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets,
                           const BoundedGeom& g, uint32_t* mode, uint32_t* lchunk, unsigned long long* lrange,
                           uint32_t* lcount, uint32_t* status, hipStream_t s);
// the mode-1 chunks' blocks into the volume, steps read from the planes launch_bb_parse validated; status |= 128 for
// a verbatim value outside 0..65535
hipError_t launch_bb_inverse(const int32_t* idx, const uint8_t* in, const unsigned long long* offsets,
                             const BoundedGeom& g, const float* dct64, const float* qtab, const uint32_t* mode,
                             uint16_t* vol, uint32_t* status, hipStream_t s);

// ---- patch-cache masks and coherence gate (mask_kernels.hip) ---------------------------------------------
constexpr int LS_MAX = 1024;        // distinct labels a patch's LDS hash set holds (exabm4d.h EXABM4D_LABEL_SET_MAX)
constexpr int SEG_STATS_K = 23;     // doubles per (patch, label) of launch_segment_stats (EXABM4D_SEG_STATS_K)
constexpr int GF_MAXR = 64;         // largest Gaussian radius (exabm4d.h EXABM4D_GAUSS_MAX_RADIUS)
enum { LBL_U8 = 0, LBL_U32 = 1, LBL_U64 = 2, LBL_I32 = 3, LBL_I64 = 4 };
struct GaussWeights {
    int radius;
    double w[GF_MAXR + 1];          // w[0] centre, w[j] = w[-j]
};
// raw: dtype 0 uint16, 1 float32; thr[batch] fp32
hipError_t launch_fg_threshold(const void* raw, int dtype, int batch, size_t n, float k, float* thr,
                               hipStream_t s);
// thr != NULL: the source is raw > thr[b] (raw_dtype as above), else the masks `in` (!= out)
hipError_t launch_dilate(const uint8_t* in, const void* raw, int raw_dtype, const float* thr, int batch,
                         int nz, int ny, int nx, int iterations, uint8_t* tmp, uint8_t* out,
                         hipStream_t s);
// the source is labels > 0 (ldtype: LBL_*)
hipError_t launch_dilate_labels(const void* labels, int ldtype, int batch, int nz, int ny, int nx, int iterations,
                                uint8_t* tmp, uint8_t* out, hipStream_t s);
// src: dtype 1 float32, 2 float64
hipError_t launch_gaussian3d(const void* src, int dtype, int batch, int nz, int ny, int nx,
                             const GaussWeights& w, double* tmp, double* out, hipStream_t s);
hipError_t launch_label_set(const void* labels, int ldtype, int batch, size_t n, unsigned long long* keys,
                            uint32_t* counts, uint32_t* n_out, uint32_t* status, hipStream_t s);
// raw: rdtype 1 float32, 2 float64; smooth may be NULL (then the raw - smooth columns are 0)
hipError_t launch_segment_stats(const void* labels, int ldtype, const void* raw, int rdtype, const double* smooth,
                                int nz, int ny, int nx, int lag, const int32_t* item_patch,
                                const unsigned long long* item_key, int items, double* out, hipStream_t s);

// ---- patch samplers (sampler_kernels.hip) ------------------------------------------------
constexpr int RASTER_BOXES = 256;   // box origins one rasteriser launch keeps in LDS (3 KiB)
struct RasterBounds {
    long long lo[3], hi[3];         // the bounding box of a launch's boxes, zyx, hi exclusive
};
// counts[b] = voxels of patch b that are set, or (iterate) have a face neighbour inside the patch that is; counts
// are zeroed on the stream first.  The source is raw > thr[b] (dtype 0 uint16, 1 float32) or a mask.
long long count_workgroups(int batch, int nz, int ny, int nx);   // the grid of the two launchers: keep below 2^31
hipError_t launch_count_above(const void* raw, int dtype, const float* thr, int batch, int nz, int ny, int nx,
                              int iterate, uint32_t* counts, hipStream_t s);
hipError_t launch_count_mask(const uint8_t* mask, int batch, int nz, int ny, int nx, int iterate, uint32_t* counts,
                             hipStream_t s);
// out[b][p - starts[b]] = 1 for every point p (int32 zyx triples) inside box b of nbox <= RASTER_BOXES boxes;
// pts, starts and out are device arrays, out is not cleared
hipError_t launch_raster_points(const int32_t* pts, size_t npts, const int32_t* starts, int nbox, int nz, int ny,
                                int nx, const RasterBounds& bb, uint8_t* out, hipStream_t s);
hipError_t launch_or_bytes(const uint8_t* in, size_t total, uint8_t* out, hipStream_t s);   // out |= in, 0 / 1 bytes

// ---- validation scoring (validate_kernels.hip) -------------------------------------------
constexpr int VAL_K = 16;           // doubles per patch (exabm4d.h EXABM4D_EVAL_K)
constexpr int VAL_MAX_SPLITS = 64;  // most statistics workgroups per patch
// row columns (exabm4d.h): 0..5 are those of launch_masked_stats
enum { VAL_MED = 6, VAL_MAD = 7, VAL_THR = 8, VAL_RAW_LO = 9, VAL_RAW_HI = 10, VAL_PRED_LO = 11, VAL_PRED_HI = 12,
       VAL_PRED_NAN = 13, VAL_RAW_NAN = 14, VAL_TARGET_NAN = 15 };
struct ValRanks {
    uint32_t r[4];                  // 0-based: the two median ranks, then the two percentile ranks
};
size_t validate_partials_bytes(int batch, size_t n);
// pred / raw / target: dtype 0 uint16, 1 float32, (batch, n) each; mask (batch, n) bytes; rows[batch][VAL_K]
hipError_t launch_validate_batch(const void* pred, int pred_dtype, const void* raw, int raw_dtype,
                                 const void* target, int target_dtype, const uint8_t* mask, int batch, size_t n,
                                 double k, const ValRanks& rk, double* partials, double* rows, hipStream_t s);

// ---- region reads of a chunk store (region_kernels.hip) ----
// A decoded chunk in the pool: exabm4d_box_src of exabm4d.h, field for field.
struct BoxSrc {
    unsigned long long base, stride_y, stride_z;    // elements
    int32_t z0, y0, x0;                             // origin in the array
    int32_t ez, ey, ex;                             // extent
};
// out[n][z][y][x] (uint16, or fp32 = value - offset) <- the first source of lists[n][0..per_box) (-1: unused) that
// holds voxel starts[n] + (z, y, x), else the fill.  srcs, lists and starts are device arrays; the caller has checked
// that every source lies inside the pool.
hipError_t launch_gather_boxes(const uint16_t* pool, const BoxSrc* srcs, const int32_t* lists, int per_box,
                               const int32_t* starts, int nbox, int bz, int by, int bx, int out_f32, float offset,
                               float fill_f32, uint16_t fill_u16, void* out, hipStream_t s);

// ---- region writes of a chunk store (region_kernels.hip) ----
// The gather's mirror: every voxel of every destination dsts[d] (a region of `pool`) takes the value of the LAST box
// of lists[d][0..per_dst) (-1: unused) that holds it, read from `src` where boxes[k] says; a voxel no listed box
// holds is not written.  kind: SCATTER_U16 (uint16 -> uint16), SCATTER_F32 (fp32 -> uint16 as rint(clamp(v + offset,
// 0, 65535))), SCATTER_U8 (bytes -> bytes).  row0[d] = the rows (ez * ey) of the destinations before d, row0[ndst] =
// rows.  boxes, dsts, row0 and lists are device arrays; the caller has checked that every record lies inside its
// buffer and that the destinations do not overlap.
enum { SCATTER_U16 = 0, SCATTER_F32 = 1, SCATTER_U8 = 2 };
hipError_t launch_scatter_boxes(const void* src, int kind, const BoxSrc* boxes, const BoxSrc* dsts,
                                const unsigned long long* row0, int ndst, const int32_t* lists, int per_dst,
                                unsigned long long rows, float offset, void* pool, hipStream_t s);

// ---- label codec (label_codec_kernels.hip) ------------------------------------------
constexpr uint32_t LB_MAGIC = 0x424C5845u;      // "EXLB", little-endian
constexpr int LB_HEADER = 32;                   // bytes of a stream's header; the block table follows
constexpr uint32_t LB_ST_MALFORMED = 1u;        // status bits of the decoders: a header or table entry was rejected,
constexpr uint32_t LB_ST_CLAMPED = 2u;          // a palette index >= k was clamped
struct LabelGeom {
    int ts;                  // element bytes: 4 (uint32) or 8 (uint64)
    int nz, ny, nx;          // volume
    int cz, cy, cx;          // chunk shape, clamped to the volume
    int gz, gy, gx;          // chunks per axis
    int nchunks;
    int nb;                  // 8^3 blocks of a full chunk: the stride of a chunk in the per-block scratch
};
int make_label_geom(int ts, int nz, int ny, int nx, int cz, int cy, int cx, LabelGeom& g);
size_t label_volume_bound(const LabelGeom& g);
// units, blockoff: nchunks * g.nb words of scratch each; sizes[nchunks], offsets[nchunks + 1], totals[2] as
// launch_codec_scan makes them; out == nullptr stops after the sizes
hipError_t launch_label_encode(const void* vol, const LabelGeom& g, uint32_t* units, uint32_t* blockoff, uint32_t* sizes,
                               unsigned long long* offsets, unsigned long long* totals, uint8_t* out, hipStream_t s);
// Never reads outside [in, in + in_bytes) nor writes outside the volume, whatever the bytes; *status |= LB_ST_*
hipError_t launch_label_decode(const uint8_t* in, size_t in_bytes, const unsigned long long* offsets, const LabelGeom& g,
                               void* vol, uint32_t* status, hipStream_t s);
// A coded chunk in the container: exabm4d_label_src of exabm4d.h, field for field.
struct LabelChunkSrc {
    unsigned long long offset, bytes;               // of its stream in the container
    int32_t z0, y0, x0;                             // origin in the array
    int32_t ez, ey, ex;                             // extent
};
// out[n][z][y][x] <- the label at starts[n] + (z, y, x), 0 outside the array.  lists[n] holds the chunks box n
// touches, in raster order of its chunk range, as rows of srcs; the caller has checked every record against the
// container and every list against the geometry.  *status |= LB_ST_*
hipError_t launch_label_gather(const uint8_t* data, int ts, const LabelChunkSrc* srcs, const int32_t* lists, int per_box,
                               const int32_t* starts, int nbox, int bz, int by, int bx, const int* shape,
                               const int* chunk, void* out, uint32_t* status, hipStream_t s);

}  // namespace exabm4d
