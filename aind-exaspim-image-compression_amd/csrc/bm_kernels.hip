// bm_kernels.hip -- 3-D block matching (SURVEY.md section 8 row a-B1).
//
// No reference source exists for this arithmetic (the reference calls the closed bm4d wheel,
// machine_learning/data_handling.py:332); the spec is DESIGN.md section 3 and the checker is
// oracle/exabm4d_oracle.c:orc_blockmatch.
//
// Distance: a block is 2x2x2 cells of 4^3 voxels.  cell SSD = 64-term fmaf chain
// in (z,y,x) raster order from +0; block SSD = pairwise tree over the 8 cells.  Cell SSDs of
// grid-aligned cells are shared by the 8 reference blocks that contain the cell, which is what
// bm_tile_kernel exploits: one lane owns one cell, cell sums go through LDS, one lane owns one
// reference block's running top-16 list.
#include "exabm4d_kernels.h"
#ifdef EXABM4D_BM_STAMPS
#define KERNEL_STAMPS
#endif
#include "kernel_stamps.h"
#include <type_traits>
#include <utility>

namespace exabm4d {

#ifdef EXABM4D_BM_STAMPS
// Diagnostic build only: per-phase cycle sums (s_memtime) of bm_tile16_kernel, accumulated over all waves.
// Slots: 0 top wait, 1 wait for the cell's own plane, 2 wait in front of the window reads, 3 accumulate,
// 4 exchange barriers, 5 selection, 6 carry waits (the poll and the tile's last drain), 7 wave lifetime.
__device__ unsigned long long g_bm_stamps[8];
// Slot 4 again, kept apart: [barrier of the (dz, pass): 2 round + (0 in front of / 1 behind the selection)][wave cz].
// The wave that arrives last at a barrier waits least in it.  Sized for the largest geometry (three rounds, twelve
// waves); a geometry with fewer leaves the rest zero.
constexpr int BM_STAMP_BARRIERS = 6, BM_STAMP_WAVES = 12;
__device__ unsigned long long g_bm_barrier_stamps[BM_STAMP_BARRIERS][BM_STAMP_WAVES];
#endif

// ------------------------------------------------------------------------------------------------
// Tile kernel: 512 lanes = 8x8x8 cells; tiles overlap by one cell in y and x so a tile yields 7x7
// grid-aligned reference blocks per layer, and 7 layers -- or 8 with the carry between tiles (CARRY below).
// ------------------------------------------------------------------------------------------------
// 16-byte load from a 4-byte aligned address (gfx950 global loads need only dword alignment;
// hipcc emits global_load_dwordx4 for this type).
struct __attribute__((packed, aligned(4))) float4u {
    float x, y, z, w;
};
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index can be an asm immediate
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

constexpr int TCZ = 8;       // cell layers per tile = waves per workgroup (the integer kernel: TileShape16::LAYERS)
constexpr int NE = 6;        // dy values per pass (two passes: dy = -5..0 and 1..6, 6 is masked)
constexpr int NSTEP = SWIN * 2 * 4;             // (dz, pass, z) steps
// A wave is one z-layer of TCY x TCX cells (64 lanes).  8 x 8 is the shape for volumes; 4 x 16
// tiles a 64^3 patch (15 reference positions per axis) exactly in x (15) and y (5 x 3), where the
// cube needs 3 x 3 tiles of 7 x 7 positions for the same 15 x 15.  The tile plan is common to the
// float and the integer kernel (bm_plan); their shapes add how a plane is staged.
template <int TCY_, int TCX_>
struct TilePlan {
    static constexpr int TCY = TCY_, TCX = TCX_;
    static constexpr int TRY = TCY - 1, TRX = TCX - 1;      // reference blocks per tile edge
    static constexpr int PROWS = 4 * (TCY - 1) + 3 + NE;    // staged rows: 4*cy + y + e (37 / 21)
    static_assert(TCY * TCX == 64, "one wave per cell layer");
};
template <int TCY_, int TCX_>
struct TileShape : TilePlan<TCY_, TCX_> {
    using Plan = TilePlan<TCY_, TCX_>;
    static constexpr int PCOLS = 4 * (TCX_ - 1) + 16;       // staged columns: 4*cx + 0..15 (44 / 76)
    // row stride in floats.  8 x 8: 56 = 8 (mod 16) makes the b128 window reads of the two cell
    // rows that share 16 lanes conflict-free; 4 x 16: 16 lanes are one cell row, any stride does.
    static constexpr int PSTR = TCX_ == 8 ? 56 : PCOLS;
    static constexpr int PCH = PSTR / 4;                    // 16-byte chunks per staged row
    static constexpr int NDMA = (Plan::PROWS * PCH + 63) / 64;    // LDS-DMA instructions per plane
    // floats per plane buffer: the staged rows (the tail of the last LDS-DMA instruction is masked off)
    // or the cell-sum exchange, 33 sums x 64 cells + the y-neighbour overhang of the last row
    static constexpr int PLANE = (Plan::PROWS * PSTR + 3) / 4 * 4;
    static constexpr int PBUF = PLANE > 2144 ? PLANE : 2144;
    static_assert(PCOLS % 4 == 0 && PSTR % 4 == 0, "whole 16-byte chunks");
};

// CARRY (round 3).  A reference block is two cell layers, so a tile of eight cell layers gives seven
// reference layers and every eighth layer is computed twice (as the top layer of a tile and as the
// bottom layer of the next): 37 tiles for the 255 reference layers of a 1024^3 volume.  With the carry
// a tile advances by EIGHT layers: wave w computes cell layer L = 8 tz + w and owns the reference layer
// L - 1 -- its lower cells are wave w - 1's sums (LDS), and for wave 0 they are the sums wave 7 of the
// tile BELOW formed, which travel through global memory: [2][columns][22 (dz, pass)][2 rounds][33 x 64],
// a slot per column and tile parity.  `done[column]` (tiles finished) orders producer and consumer: waves 0
// and 7 wait for done >= tz before they read / overwrite a slot.
// ORDER (round 4): a workgroup does not take its tile from blockIdx -- HIP does not promise that workgroups
// start in id order -- but from a TICKET: thread 0 draws `atomicAdd(ticket, 1)` when the workgroup starts,
// and the ticket goes through the slab-order map (xcd_slab_sync; one ticket sequence per XCD, launch_position).
// The producer of a tile's carry is the same slab position one slab earlier: q tickets back in the same
// sequence.  A smaller ticket of a sequence has been drawn earlier, so its
// workgroup is resident or finished, and it in turn only waits for a smaller ticket still: by induction
// every wait ends, whatever order the hardware dispatches in (the look-back argument of rocPRIM's scans).
// The poll is bounded all the same (CARRY_POLL_LIMIT, seconds): on expiry the wave raises bit 0 of the
// context's status word (host-visible), goes on WITHOUT a valid carried layer -- that launch's tables are
// void -- and the host reports EXABM4D_ERR_HIP at its next synchronisation and switches the carry off for
// the context (exabm4d_api.hip: check_async_status); never a hang.  All carry traffic is system-scope (stores written through,
// loads and the LDS-DMA prefetch with sc0 sc1): no assumption about which XCD's L2 a tile runs on.  Wave 0
// fetches a (dz, pass)'s whole slot by LDS-DMA one plane ahead of its use: no registers, no wait in
// front of the exchange barriers.  The same sums enter the same adds: tables are unchanged.
// SLOT LAYOUT.  The slot of a (dz, pass) is linear [dy row e = 0 .. 5][d = 0 .. 10][64 cells], 2 * CARRY_ROUND
// elements, in global memory and in lower0 alike: dy row e lies at e * SWIN * 64 however many rows an exchange round
// publishes.  The 8-layer tiles exchange three rows per round (two rounds, the second at CARRY_ROUND), the integer
// kernel's 12-layer tiles two rows (three rounds, at 0, 2 and 4 * SWIN * 64; TileShape16::XROWS): the carrying wave
// stores and wave 0 reads round e0 at e0 * SWIN * 64 in both, so the slot's size, the prefetch of a whole slot and
// the done[] protocol do not depend on the round size (tests/test_bm_layers_gpu.py forces the carry in both).
constexpr int CARRY_ROUND = (NE / 2) * SWIN * 64;                 // half a (dz, pass): three dy rows of 11 sums x 64 cells
constexpr int CARRY_TILE = (NSTEP / 4) * 2 * CARRY_ROUND;         // one tile's top layer: 22 (dz, pass) x 6 dy rows
struct Carry {
    int on;                  // 1: tiles advance by TCZ cell layers and carry their top layer
    int strip;               // tile order inside a slab: strips of this many tile rows, column-major (0 = raster)
    uint32_t* buf;           // [2][columns][CARRY_TILE]
    int* done;               // [columns]: tiles of the column that have finished (zeroed per launch)
    int* ticket;             // the launch's eight ticket counters (zeroed per launch), see ORDER above and launch_position
    unsigned* status;        // host-visible status word of the context: bit 0 = a carry wait ran out
    int fault;               // debug option "bm_carry_fault": every wait counts as run out (tests of the error path)
};
constexpr int CARRY_POLL_LIMIT = 1 << 23;       // x s_sleep(32) = 2048 cycles: ~7 s at 2.4 GHz
// The whole slot of one (dz, pass) into `dst` (2 * CARRY_ROUND elements, linear): 16 full 1 KB transfers
// and one of 512 bytes.
template <class T, class D>
__device__ __forceinline__ void carry_prefetch(const T* src, D* dst, int lane) {
    static_assert(2 * CARRY_ROUND == 16 * 256 + 128, "a slot = 16.5 KB");
#pragma unroll
    for (int i = 0; i < 16; i++)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 256 * i + 4 * lane),
                                         (__attribute__((address_space(3))) void*)(dst + 256 * i), 16, 0, 17);
    if (lane < 32)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 4096 + 4 * lane),
                                         (__attribute__((address_space(3))) void*)(dst + 4096), 16, 0, 17);
}
__device__ __forceinline__ void carry_wait_for(const int* done, int tiles, int lane, const Carry& carry) {
    if (lane == 0) {
        int polls = carry.fault ? CARRY_POLL_LIMIT : 0;
        while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < tiles) {
            if (++polls > CARRY_POLL_LIMIT) {
                __hip_atomic_fetch_or(carry.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            __builtin_amdgcn_s_sleep(32);
        }
        // (the forced fault must not depend on a race with the producer)
        if (carry.fault) __hip_atomic_fetch_or(carry.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// The workgroup's position in the launch order: its ticket when tiles carry (see ORDER), else its id.
// EIGHT ticket counters, one per XCD sequence of the slab order (position = 8 j + c: XCD c's j-th tile): a
// workgroup draws from the counter of the XCD it runs on (HW_REG_XCC_ID), so that the tiles an XCD works on
// stay neighbours in ITS L2 -- one global counter handed consecutive tickets to whichever XCD asked first
// and cost block matching its cache sharing (PMC: 43 -> 151 GB and 152 -> 280 GB per 1024^3 launch,
// 116 -> 120-128 ms for the fp32 kernel).  A launch has exactly `quota` positions per sequence; should the
// hardware give an XCD more workgroups than that, the surplus ones draw from the other sequences in turn
// (8 * quota workgroups, 8 * quota positions: everybody finds one, every position is taken).  The order
// argument holds per counter: a tile's producer is ticket j - q of the SAME counter, drawn earlier.
__device__ __forceinline__ int launch_position(const Carry& carry, int quota) {
    if (!carry.on) return (int)blockIdx.x;
    __shared__ int s_pos;
    if (threadIdx.x == 0) {
        const int xcc = (int)(__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 7);     // HW_REG_XCC_ID
        int pos = -1;
        for (int k = 0; k < 8 && pos < 0; k++) {
            const int c = (xcc + k) & 7;
            const int j = __hip_atomic_fetch_add(carry.ticket + c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (j < quota) pos = 8 * j + c;
        }
        s_pos = pos;      // (-1 cannot happen: as many workgroups as positions; treated as padding)
    }
    __syncthreads();
    return s_pos;
}

// ------------------------------------------------------------------------------------------------
// What both tile kernels share: which tile a workgroup computes, how a reference lane admits a candidate
// to its top-16 list and how it writes the list to the table.
// ------------------------------------------------------------------------------------------------
// Tile order.  Slab order (xcd_q != 0): one slab = the tiles of ONE tz of all batch elements, all XCDs
// inside it (xcd_slab_sync); a column is (batch element, ty, tx).  Otherwise every XCD walks its own
// contiguous range of a batch element's tiles (blockIdx.y = batch element).
struct TileId {
    int tz, col, cols;       // z tile, its column and the launch's columns
    int bi, ty, tx;          // the column's batch element and (y, x) tile
};
// false: the workgroup is padding of the slab order and returns
__device__ __forceinline__ bool tile_id(TileId& t, int tiles_y, int tiles_x, int xcd_q, int nbatch,
                                        const Carry& carry) {
    const int per = tiles_y * tiles_x;
    t.cols = per * nbatch;
    if (xcd_q) {
        const int lp = launch_position(carry, (int)(gridDim.x >> 3));
        const int s = lp < 0 ? -1 : xcd_slab_sync(lp, t.cols, xcd_q);
        if (s < 0) return false;
        t.tz = s / t.cols;
        t.col = s - t.tz * t.cols;
    } else {
        const int s = xcd_contiguous(blockIdx.x, gridDim.x);
        t.tz = s / per;
        t.col = (int)blockIdx.y * per + (s - t.tz * per);
    }
    t.bi = t.col / per;
    const int pos = t.col - t.bi * per;
    int ty, tx;             // (locals: fields the two branches write in different orders end up in scratch)
    if (carry.strip) {      // strips of `strip` tile rows, column-major inside a strip: concurrent tiles form a compact patch
        const int sidx = pos / (carry.strip * tiles_x), r = pos - sidx * (carry.strip * tiles_x);
        const int h = min(carry.strip, tiles_y - sidx * carry.strip);
        tx = r / h;
        ty = sidx * carry.strip + (r - tx * h);
    } else {
        ty = pos / tiles_x;
        tx = pos - ty * tiles_x;
    }
    t.ty = ty;
    t.tx = tx;
    return true;
}

// A reference lane's running top-16 list `list`, `thr` = min(list[15], keymax): a key below it enters the list.
// Admits candidate `code` at the distance whose fp32 bits are `sbits`.
__device__ __forceinline__ void list_admit(uint32_t (&list)[MAXG], uint32_t& thr, uint32_t keymax, uint32_t sbits,
                                           uint32_t code, bool valid) {
    uint32_t key = (sbits & KEY_DMASK) | code;
    key = valid ? key : KEY_EMPTY;
    // thr = min(16th best so far, admission bound): one compare decides
    if (__any(key < thr)) {
        const uint32_t kins = key < thr ? key : KEY_EMPTY;
        list_insert_inplace(list, kins);
        thr = min(list[MAXG - 1], keymax);
    }
}
// The reference block's 16 keys of the table.
__device__ __forceinline__ void list_store(uint32_t* out, uint32_t (&list)[MAXG]) {
    // never empty: a block with an infinity or a NaN in it has no admissible distance, not
    // even to itself; it forms the one-block group of key 0, so that every key downstream names a block
    list[0] = list[0] == KEY_EMPTY ? 0u : list[0];
#pragma unroll
    for (int k = 0; k < MAXG; k += 4) {
        uint4 v = make_uint4(list[k], list[k + 1], list[k + 2], list[k + 3]);
        *reinterpret_cast<uint4*>(out + k) = v;
    }
}

// Each WAVE (= one z-layer of 8x8 cells) streams the candidate planes it needs through its own
// pair of LDS buffers: for a fixed dz and a pass of NE dy values, plane z+dz of the volume
// (37 rows x 44 columns around the tile) is staged once and serves all 4 x NE x 11 (row, dy, dx)
// combinations of every cell of the wave.  Interior tiles stage with LDS-DMA
// (global_load_lds_dwordx4: no registers, one step ahead of the arithmetic); tiles at an x edge
// of the volume stage synchronously with per-element clamping.  The search window is therefore
// read from L2/HBM 2 x 11 times per plane instead of 121 x 4 times per row (measured before:
// 1.8 TB of fabric traffic per 1024^3 launch at 7 TB/s -- bandwidth-bound on re-reads).
// The cell-sum exchange buffer aliases the waves' current plane buffers (each wave publishes the
// sums of its own 64 cells in its own buffer once its reads of the plane are done).
template <class TS>
__global__ __launch_bounds__(512) void bm_tile_kernel(const float* __restrict__ vol_all, VolGeom g,
                                                      uint32_t keymax,
                                                      uint32_t* __restrict__ keys_all, int tiles_y,
                                                      int tiles_x, int guarded, int xcd_q, int nbatch, Carry carry) {
    constexpr int TCX = TS::TCX, TRX = TS::TRX, TRY = TS::TRY, PROWS = TS::PROWS,
                  PCOLS = TS::PCOLS, PSTR = TS::PSTR, PCH = TS::PCH, NDMA = TS::NDMA, PBUF = TS::PBUF;
    __shared__ __align__(16) float pbuf_all[TCZ][2][PBUF];
    __shared__ __align__(16) float lower0[2 * CARRY_ROUND + 64];   // wave 0's lower cell layer (from the carry), both rounds

    TileId id;
    if (!tile_id(id, tiles_y, tiles_x, xcd_q, nbatch, carry)) return;
    const int tz = id.tz, col = id.col, cols = id.cols, bi = id.bi, ty = id.ty, tx = id.tx;
    const float* __restrict__ vol = vol_all + (size_t)bi * (size_t)g.nvox;
    uint32_t* __restrict__ keys = keys_all + (size_t)bi * (size_t)g.nref * MAXG;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int cx = lane % TCX, cy = lane / TCX, cz = __builtin_amdgcn_readfirstlane(tid >> 6);   // cz == wave index
    const int ix = TRX * tx + cx, iy = TRY * ty + cy;                 // cell == ref index in y, x

    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;

    // cell layers a tile advances by (CARRY above); this tile's column and its two carry slots
    const int Ls = (carry.on ? TCZ : TCZ - 1) * tz;
    const float* carry_rd = reinterpret_cast<const float*>(carry.buf) + ((size_t)((tz + 1) & 1) * cols + col) * CARRY_TILE;
    float* carry_wr = reinterpret_cast<float*>(carry.buf) + ((size_t)(tz & 1) * cols + col) * CARRY_TILE;
    int* done_col = carry.done + col;

    // Cell origin; cells beyond the volume are clamped inside it (their sums are never used).
    const int qy = min(STEP * iy, g.ny - STEP), qx = min(STEP * ix, g.nx - STEP);
    // Tile origin (voxels) of the staged window; wave-uniform.
    const int Y0 = STEP * TRY * ty, X0 = STEP * TRX * tx - RAD;
    // Whole staged column range inside the volume?  (wave-uniform; edge tiles clamp per element.)
    // `guarded`: the volume is one of the library's own buffers, with >= 256 bytes of mapped memory
    // on either side.  Columns outside the volume then need no clamping at all: they only ever
    // enter the distances of candidates that lie partly outside the volume, which `valid` masks
    // (a block inside the volume has all its columns inside), so x-edge tiles can take the
    // LDS-DMA path too and read whatever lies beyond the row ends.
    const bool xin = guarded || ((X0 >= 0) && (X0 + PCOLS - 1 <= g.nx - 1));

    const bool ref_yx = cx < TRX && cy < TRY && iy < g.ay && ix < g.ax;
    const int ry = STEP * iy, rx = STEP * ix;

    // bit d set iff candidate displacement dx = d - 5 keeps the block inside the volume
    uint32_t xmask = 0;
#pragma unroll
    for (int d = 0; d < SWIN; d++)
        xmask |= ((rx + d - RAD >= 0) && (rx + d - RAD <= g.nx - BLK)) ? (1u << d) : 0u;

    const bool yin = (Y0 - RAD >= 0) && (Y0 + 1 + PROWS - 1 <= g.ny - 1);
    do {   // once; `break` = an idle wave skips the tile's work, not the barriers and the tail below
    const int L = Ls + cz;                             // this wave's cell layer
    const bool active = L <= g.az;
    const int iz = L - 1;                              // the reference layer it owns (lower cells: wave cz - 1)
    const int qz = min(STEP * L, g.nz - STEP);
    const int Z0 = STEP * L;
    const bool lower_carried = carry.on && cz == 0 && tz > 0;          // the lower layer is the tile below's top layer
    const bool carries = carry.on && cz == TCZ - 1 && L + 1 <= g.az;   // ... and this wave's sums are the next tile's
    const bool ref_ok = ref_yx && active && (cz > 0 || lower_carried);
    if ((lower_carried || carries) && tz > 0) carry_wait_for(done_col, tz, lane, carry);
    const int rz = STEP * iz;

    uint32_t list[MAXG];
#pragma unroll
    for (int k = 0; k < MAXG; k++) list[k] = KEY_EMPTY;
    uint32_t thr = keymax;       // min(list[15], keymax): a key below it enters the list

    auto step_plane = [&](int step, int& dylo) -> const float* {
        const int z = step & 3, pass = (step >> 2) & 1, dz = (step >> 3) - RAD;
        dylo = pass == 0 ? -RAD : 1;
        const int pz = min(max(Z0 + z + dz, 0), g.nz - 1);
        return vol + (size_t)pz * sz;
    };
    // LDS-DMA of one plane into buffer `dst`: instruction i writes floats [256 i, 256 i + 256)
    // linearly, lane l the 16 bytes at chunk p = 64 i + l = (row p / 14, column chunk p % 14);
    // chunks beyond column 10 or row 36 are padding and re-read a valid address.
    // Tiles whose staged rows all lie inside the volume in y (all but the first and last tile row):
    // the row of a chunk needs no clamp, so its source is a wave-uniform base (plane, first row,
    // first column) plus a lane constant r * sy + 4 q -- eight instructions per DMA instead of the
    // thirty of the clamped form (a fifth of a step's instructions went into these addresses).
    auto issue_dma = [&](int step, float* dst) {
        int dylo;
        const float* plane = step_plane(step, dylo);
        int l = lane;
        asm volatile("" : "+v"(l));          // keeps the 9 (row, column) pairs out of registers
        if (yin) {
            const float* base = plane + (ptrdiff_t)(Y0 + dylo) * (ptrdiff_t)sy + X0;
#pragma unroll
            for (int i = 0; i < NDMA; i++) {
                const unsigned p = 64u * i + (unsigned)l;
                const unsigned r0 = (p * (65536u / PCH + 1u)) >> 16;          // p / PCH for p < 2^12
                const unsigned r = min(r0, (unsigned)(PROWS - 1));
                const unsigned q = min(p - r0 * PCH, (unsigned)(PCOLS / 4 - 1));
                const float* src = base + (r * (unsigned)sy + 4u * q);
                if (64 * i + 64 <= PROWS * PCH || p < (unsigned)(PROWS * PCH))       // chunks past the last row stay unwritten
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void*)src,
                        (__attribute__((address_space(3))) void*)(dst + 256 * i), 16, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NDMA; i++) {
            const int p = 64 * i + l;
            const int r = min(p / PCH, PROWS - 1), q = min(p % PCH, PCOLS / 4 - 1);
            const int yy = min(max(Y0 + dylo + r, 0), g.ny - 1);
            const float* src = plane + (size_t)yy * sy + (X0 + 4 * q);
            if (64 * i + 64 <= PROWS * PCH || p < PROWS * PCH)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)src,
                    (__attribute__((address_space(3))) void*)(dst + 256 * i), 16, 0, 0);
        }
    };
    auto stage_edge = [&](int step, float* dst) {               // edge tiles: clamp per element
        int dylo;
        const float* plane = step_plane(step, dylo);
        for (int c = lane; c < PROWS * PCOLS; c += 64) {
            const int r = c / PCOLS, q = c - r * PCOLS;
            const int yy = min(max(Y0 + dylo + r, 0), g.ny - 1);
            const int xx = min(max(X0 + q, 0), g.nx - 1);
            dst[r * PSTR + q] = plane[(size_t)yy * sy + xx];
        }
    };

    // A wave whose cell layer lies beyond the last one any reference block uses (layers 0 .. az)
    // has nothing to contribute -- the last z tile of a 64^3 patch needs 2 of its 8 layers -- and
    // only keeps the workgroup's barrier count: four per (dz, pass).
    if (!active) {
        for (int i = 0; i < (NSTEP / 4) * 4; i++) __syncthreads();
        break;
    }

    if (xin)
        issue_dma(0, pbuf_all[cz][0]);
    else
        stage_edge(0, pbuf_all[cz][0]);

    float acc[NE][SWIN];
#pragma unroll
    for (int e = 0; e < NE; e++)
#pragma unroll
        for (int d = 0; d < SWIN; d++) acc[e][d] = 0.0f;

#pragma unroll 1
    for (int step = 0; step < NSTEP; step++) {
        const int z = step & 3, pass = (step >> 2) & 1, dz = (step >> 3) - RAD;
        const int dylo = pass == 0 ? -RAD : 1;
        float* cur = pbuf_all[cz][step & 1];
        float* nxt = pbuf_all[cz][(step + 1) & 1];

        // this step's plane has landed (DMA counts in vmcnt) ...
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // own cell plane z (16 values; L1-resident after the first pass)
        float A[16];
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const float4u t4 = *reinterpret_cast<const float4u*>(
                vol + (size_t)(qz + z) * sz + (size_t)(qy + y) * sy + qx);
            A[4 * y] = t4.x;
            A[4 * y + 1] = t4.y;
            A[4 * y + 2] = t4.z;
            A[4 * y + 3] = t4.w;
        }
        // ... and the next plane starts flying while this one is consumed.  The A loads are
        // drained first: vmcnt retires in order and hipcc waits vmcnt(0) for A after the
        // (conditional) DMA block, which would expose the whole DMA latency every step.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (xin && step + 1 < NSTEP) issue_dma(step + 1, nxt);
        if (lower_carried && z == 2) carry_prefetch(carry_rd + (size_t)(step >> 2) * 2 * CARRY_ROUND, lower0, lane);

        // ---- accumulate: row rp = y + e of the cell's window -----------------------------------
        // (Plain LDS reads, in front of the first of which hipcc drains the DMA just issued -- see
        // bm_tile16_kernel.  Its hand-waited rows -- four asm ds_read_b128 and an lgkmcnt(0) per row -- were built
        // here too: 249 -> 256 registers and 18 / 20 spilled ones, 76 / 84 bytes of scratch; not taken.)
        {
            const float* wrow = cur + (4 * cy) * PSTR + 4 * cx;
            float4 wq[4], wn[4];
#pragma unroll
            for (int j = 0; j < 4; j++) wq[j] = *reinterpret_cast<const float4*>(wrow + 4 * j);
#pragma unroll
            for (int rp = 0; rp < 3 + NE; rp++) {
                // one-row lookahead; the fence keeps hipcc from hoisting all nine rows' loads
                // (and their 144 registers) to the top of the plane
                if (rp + 1 < 3 + NE) {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        wn[j] = *reinterpret_cast<const float4*>(wrow + (rp + 1) * PSTR + 4 * j);
                }
                asm volatile("" ::: "memory");
                const float w[16] = {wq[0].x, wq[0].y, wq[0].z, wq[0].w, wq[1].x, wq[1].y,
                                     wq[1].z, wq[1].w, wq[2].x, wq[2].y, wq[2].z, wq[2].w,
                                     wq[3].x, wq[3].y, wq[3].z, wq[3].w};
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    const int e = rp - y;
                    if (e >= 0 && e < NE) {
#pragma unroll
                        for (int x = 0; x < 4; x++) {
                            const float a = A[4 * y + x];
#pragma unroll
                            for (int d = 0; d < SWIN; d++) {
                                const float t = a - w[d + x];
                                acc[e][d] = fmaf(t, t, acc[e][d]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) wq[j] = wn[j];
            }
        }
        asm volatile("" ::: "memory");

        if (z == 3) {
            // ---- cell sums -> LDS -> reference lanes: combine 8 cells, build keys, top-16 ------
            // exchange slot of cell (wave w, local l), displacement d: pbuf_all[w][cur][64 d + l]
            const bool vz = (rz + dz >= 0) && (rz + dz <= g.nz - BLK);
            float* mine = cur + lane;
            const float* up_w = cur + lane;                                  // own cells: the upper layer
            // the lower layer: wave cz - 1's sums; for wave 0 the previous block's top layer
            const float* lo_w = (cz > 0 ? pbuf_all[max(cz - 1, 0)][step & 1] : lower0) + lane;
            float* cslot = carry_wr + (size_t)((step >> 2) * 2) * CARRY_ROUND + lane;
            // NE / 2 dy values per round (33 sums per cell fit the 36 slots of a plane buffer):
            // two barrier pairs per pass instead of six.  Each cell lane first adds its
            // x-neighbour's sum (DPP row_shl:1, no LDS), so a reference lane reads 4 values per
            // candidate instead of 8: S = ((c000+c001)+(c010+c011)) + ((c100+c101)+(c110+c111)).
#pragma unroll
            for (int e0 = 0; e0 < NE; e0 += NE / 2) {
#pragma unroll
                for (int e = e0; e < e0 + NE / 2; e++)
#pragma unroll
                    for (int d = 0; d < SWIN; d++) {
                        const float right = __int_as_float(__builtin_amdgcn_update_dpp(
                            0, __float_as_int(acc[e][d]), 0x101 /* row_shl:1 */, 0xF, 0xF, true));
                        mine[64 * ((e - e0) * SWIN + d)] = acc[e][d] + right;
                    }
                __syncthreads();
                if (ref_ok) {
#pragma unroll
                    for (int e = e0; e < e0 + NE / 2; e++) {
                        const int dy = dylo + e;
                        if (dy <= RAD) {                   // dy = 6 of the second pass is a dummy
                            const bool vzy = vz && (ry + dy >= 0) && (ry + dy <= g.ny - BLK);
                            const uint32_t cbase =
                                1u + (uint32_t)(((dz + RAD) * SWIN + (dy + RAD)) * SWIN);
                            const bool self_row = (dz == 0) && (dy == 0);
#pragma unroll
                            for (int d = 0; d < SWIN; d++) {
                                const float* c0 = lo_w + (cz == 0 && e0 ? CARRY_ROUND : 0) + 64 * ((e - e0) * SWIN + d);
                                const float* c1 = up_w + 64 * ((e - e0) * SWIN + d);
                                // S = (c0[0] + c0[TCX]) + (c1[0] + c1[TCX]) as three plain adds: left
                                // to the SLP vectoriser this becomes two packed adds, three moves and
                                // two wait states
                                float s0 = c0[0] + c0[TCX];
                                asm("" : "+v"(s0));        // (an opaque use keeps the two sums apart)
                                const float s1 = c1[0] + c1[TCX];
                                const float S = s0 + s1;
                                const uint32_t code = (d == RAD && self_row) ? 0u : cbase + d;
                                const bool valid = vzy && ((xmask >> d) & 1u);
                                list_admit(list, thr, keymax, __float_as_uint(S), code, valid);
                            }
                        }
                    }
                }
                __syncthreads();
                if (carries) {
                    // the top wave's sums are the next block's lowest layer (read there by wave 0 in
                    // this same round, i.e. before this slot is written again)
#pragma unroll
                    for (int e = e0; e < e0 + NE / 2; e++)
#pragma unroll
                        for (int d = 0; d < SWIN; d++) {
                            const float right = __int_as_float(__builtin_amdgcn_update_dpp(
                                0, __float_as_int(acc[e][d]), 0x101 /* row_shl:1 */, 0xF, 0xF, true));
                            __hip_atomic_store(cslot + (e0 ? CARRY_ROUND : 0) + 64 * ((e - e0) * SWIN + d), acc[e][d] + right,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                }
            }
#pragma unroll
            for (int e = 0; e < NE; e++)
#pragma unroll
                for (int d = 0; d < SWIN; d++) acc[e][d] = 0.0f;
        }

        // edge tiles stage the next plane synchronously (all reads of `nxt` are long done)
        if (!xin && step + 1 < NSTEP) stage_edge(step + 1, nxt);
    }

    if (ref_ok) list_store(keys + ((size_t)((size_t)iz * g.gy + iy) * g.gx + ix) * MAXG, list);
    } while (false);

    if (carry.on) {
        // the tile is finished when wave 7's stores have been acknowledged and wave 0's last prefetch has landed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(done_col, tz + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------------------
// Integer tile kernel for uint16 volumes (stage-1 matching of the uint16 pipelines).
//
// The noisy volume of the uint16 entry points is `(float)v - offset`: differences of two voxels are
// exact integers, so every partial sum of the specification's fmaf chains is an integer, and as
// long as a block distance stays below 2^24 it is EXACT in fp32 -- the chain order no longer
// matters and the same number can be formed in integer arithmetic.  A candidate is admitted only
// below keymax <= 2^24 (checked by the launcher: c_match * sigma^2 * 512 < 2^24), so for every
// candidate that can enter a match table the integer sum converted to float has exactly the bits
// the float kernel produces, and everything else is rejected by both.  v_pk_sub_i16 (saturating)
// forms two differences, v_dot2_i32_i16 (saturating) squares and accumulates both: the same two
// instructions per two (voxel, displacement) pairs as the packed-fp32 form, and -- measured,
// tools/dbg/valu_rate_bench.hip -- at the same ~4.3 cycles each; what the integer form saves is
// LDS: a staged plane is half the bytes and a window row two ds_read_b64 instead of four b128.
//
// Input: the volume with every voxel XOR 0x8000 (= v - 32768 as int16), in the library's scratch
// with mapped memory around it (written next to the fp32 counts by the uint16 pipelines).  The
// bias makes the saturating int16 subtraction exact for |a - w| < 32768; a saturated difference
// squares to > 2^29 and can never be admitted.  nx must be even (4-byte aligned LDS-DMA rows).
// ------------------------------------------------------------------------------------------------
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// LAYERS: cell layers per tile = waves per workgroup, 8 or 12.  The fp32 kernel needs 249-252
// registers and stays at TCZ = 8, two waves per SIMD; the integer kernel's 166 fit three (168 at most), and its LDS
// does not stand in the way either: what made a plane buffer 2112 dwords was never the plane (PLANE_DW = 1280) but
// the cell-sum exchange of HALF a pass at a time, three dy rows of 11 sums for 64 cells.  The exchange round is
// therefore a constant of the shape, XROWS dy rows: the most whose sums fit a wave's share of the CU's 160 KB next
// to lower0 -- 3 rows for 8 waves, as before, and 2 rows for 12 (12 x 2 x 1408 dwords = 8 x 2 x 2112: the same LDS
// to the byte).  A pass of 6 / 5 rows then takes rounds of 3 + 3 / 3 + 2 rows, or of 2 + 2 + 2 / 2 + 2 + 1.
// Nothing else moves: the sums, the order of the adds and of the candidates are those of the 8-layer tile.
constexpr int LDS_CU_BYTES = 160 * 1024;
constexpr int LOWER0_DW = 2 * CARRY_ROUND + 64;           // wave 0's lower cell layer: a whole (dz, pass) + the y overhang
template <int TCY_, int TCX_, int LAYERS_ = TCZ>
struct TileShape16 : TilePlan<TCY_, TCX_> {
    using Plan = TilePlan<TCY_, TCX_>;
    static constexpr int LAYERS = LAYERS_;
    static constexpr int PCOLS = ((4 * TCX_ + 10 + 7) / 8) * 8;   // staged uint16 columns (48 / 80)
    // row stride in uint16: two cell rows of a 32-lane ds_read_b64 group must fall into different
    // 16-bank windows (8 x 8: 56 = 24 mod 32), one 16-lane cell row is 32 banks (4 x 16: 80 = 16 mod 32)
    static constexpr int PSTR = TCX_ == 8 ? 56 : 80;
    static constexpr int PCH = PSTR / 8;                          // 16-byte chunks per staged row
    static constexpr int NDMA = (Plan::PROWS * PCH + 63) / 64;
    static constexpr int PLANE_DW = NDMA * 256;                   // dwords of one plane buffer
    // dwords a wave's plane buffer may take: the CU's LDS less lower0 and the launch position, over 2 LAYERS buffers
    static constexpr int BUF_BUDGET_DW = ((LDS_CU_BYTES - 16) / 4 - LOWER0_DW) / (2 * LAYERS);
    static constexpr int XROWS_FIT = BUF_BUDGET_DW / (SWIN * 64);
    static constexpr int XROWS = XROWS_FIT < NE / 2 ? XROWS_FIT : NE / 2;     // dy rows per exchange round (3 / 2)
    static constexpr int XCH_DW = XROWS * SWIN * 64;              // cell-sum exchange: 33 / 22 sums x 64 cells
    static constexpr int PBUF = PLANE_DW > XCH_DW ? PLANE_DW : XCH_DW;
    // an upper bound, not the compiler's figure: 16 bytes stand for launch_position's 4-byte s_pos and any padding
    // (8 and 12 layers: 152 336 here, 152 324 in the code object)
    static constexpr int LDS_BYTES = (LAYERS * 2 * PBUF + LOWER0_DW) * 4 + 16;
    // Exchange rounds of a pass of `rows` dy values, and the workgroup barriers of a tile: two per round, around
    // the selection.  The waves that work and the idle waves of a column's last tile take their counts from HERE,
    // both of them: a wave that passes one barrier fewer than the others leaves them waiting for ever.
    static constexpr int rounds(int rows) { return (rows + XROWS - 1) / XROWS; }
    static constexpr int TILE_BARRIERS = SWIN * 2 * (rounds(NE) + rounds(NE - 1));
    static_assert(PCOLS <= PSTR, "staged columns fit the row");
    static_assert(XROWS >= 1 && PBUF >= PLANE_DW && PBUF >= XCH_DW, "a buffer holds a plane and an exchange round");
    static_assert(LDS_BYTES <= LDS_CU_BYTES, "one workgroup's LDS fits the CU");
    static_assert(64 * LAYERS <= 1024, "one wave per cell layer");
};

template <class TS>
__global__ __launch_bounds__(64 * TS::LAYERS) void bm_tile16_kernel(const uint16_t* __restrict__ vol_all, VolGeom g,
                                                        uint32_t keymax,
                                                        uint32_t* __restrict__ keys_all, int tiles_y,
                                                        int tiles_x, int xcd_q, int nbatch, Carry carry) {
    constexpr int TCX = TS::TCX, TRX = TS::TRX, TRY = TS::TRY, PROWS = TS::PROWS, PCOLS = TS::PCOLS,
                  PSTR = TS::PSTR, PCH = TS::PCH, NDMA = TS::NDMA, PBUF = TS::PBUF, LAYERS = TS::LAYERS,
                  XROWS = TS::XROWS;
    __shared__ __align__(16) uint32_t pbuf_all[LAYERS][2][PBUF];
    __shared__ __align__(16) uint32_t lower0[LOWER0_DW];   // wave 0's lower cell layer (from the carry), all rounds of a (dz, pass)

    TileId id;
    if (!tile_id(id, tiles_y, tiles_x, xcd_q, nbatch, carry)) return;
    const int tz = id.tz, col = id.col, cols = id.cols, bi = id.bi, ty = id.ty, tx = id.tx;
    const uint16_t* __restrict__ vol = vol_all + (size_t)bi * (size_t)g.nvox;
    uint32_t* __restrict__ keys = keys_all + (size_t)bi * (size_t)g.nref * MAXG;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int cx = lane % TCX, cy = lane / TCX, cz = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ix = TRX * tx + cx, iy = TRY * ty + cy;
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
#ifdef EXABM4D_BM_STAMPS
    unsigned long long st[8] = {}, stb[BM_STAMP_BARRIERS] = {};
    const unsigned long long tk0 = stamp();
#endif

    // cell layers a tile advances by (CARRY above); this tile's column and its two carry slots
    const int Ls = (carry.on ? LAYERS : LAYERS - 1) * tz;
    const uint32_t* carry_rd = carry.buf + ((size_t)((tz + 1) & 1) * cols + col) * CARRY_TILE;
    uint32_t* carry_wr = carry.buf + ((size_t)(tz & 1) * cols + col) * CARRY_TILE;
    int* done_col = carry.done + col;

    const int qy = min(STEP * iy, g.ny - STEP), qx = min(STEP * ix, g.nx - STEP);
    // staged window: rows Y0 + dylo ..., columns X0 ... with X0 even (one column more to the left
    // than the search needs): cell cx finds candidate column x + d of its voxel x at staged
    // column 4 cx + 1 + x + d
    const int Y0 = STEP * TRY * ty, X0 = STEP * TRX * tx - RAD - 1;
    const int ry = STEP * iy, rx = STEP * ix;
    const bool ref_yx = cx < TRX && cy < TRY && iy < g.ay && ix < g.ax;

    uint32_t xmask = 0;
#pragma unroll
    for (int d = 0; d < SWIN; d++)
        xmask |= ((rx + d - RAD >= 0) && (rx + d - RAD <= g.nx - BLK)) ? (1u << d) : 0u;

    do {   // once; `break` = an idle wave skips the tile's work, not the barriers and the tail below
    const int L = Ls + cz;                             // this wave's cell layer
    const bool active = L <= g.az;                     // cell layers 0 .. az exist
    const int iz = L - 1;                              // ... and the reference layer it owns
    const int qz = min(STEP * L, g.nz - STEP);
    const int Z0 = STEP * L;
    const bool lower_carried = carry.on && cz == 0 && tz > 0;          // the lower layer is the tile below's top layer
    const bool carries = carry.on && cz == LAYERS - 1 && L + 1 <= g.az;   // ... and this wave's sums are the next tile's
    const bool ref_ok = ref_yx && active && (cz > 0 || lower_carried);
    {
        STAMP(c0);
        if ((lower_carried || carries) && tz > 0) carry_wait_for(done_col, tz, lane, carry);
        STAMP(c1);
        STAMP_ADD(6, c0, c1);
    }
    const int rz = STEP * iz;

    uint32_t list[MAXG];
#pragma unroll
    for (int k = 0; k < MAXG; k++) list[k] = KEY_EMPTY;
    uint32_t thr = keymax;

    // The cell's own plane z = step & 3: four rows of four biased uint16 (two dwords each).  Hand-waited form:
    // loaded into `An` a step ahead of its use.  The loads are PLAIN ones: hipcc waits for them at their first
    // use, which is the top of the next step, where the plane's LDS-DMA is retired anyway.  (Inline-asm loads
    // would be hidden from its wait counts altogether, but it takes an asm load's destination for written when
    // the statement ends: built that way, it copied the destination registers to those of `A` ABOVE the
    // hand-placed wait, "=v" and "+v" operands alike, i.e. before the data had landed.)
    //
    // Step addresses.  Which row and column a lane fetches depends on the
    // lane, the tile and -- where staged rows clamp at a y edge -- the pass; what changes from step to step is the
    // plane, and that is wave-uniform.  So a lane keeps 32-bit byte offsets, computed once per tile: `doff[pass][i]`
    // for LDS-DMA chunk i, from the pass's first staged row at column X0, and `coff[y]` for its cell's four rows,
    // from row Y0.  A step forms the plane's base in scalar registers and the loads take base + zero-extended
    // offset (global_load_lds_dwordx4 v, s[]): the same addresses as before, without the per-chunk multiplies and
    // 64-bit vector adds.  Rows clamp monotonically, so no offset is negative and every one is below
    // (PROWS nx + PCOLS) 2 < 2^32 (launch_blockmatch checks).  X0 is negative in the first tile column: the base
    // may lie before the volume -- integer arithmetic on the pointer, never dereferenced as such, and the bytes
    // in front of the volume that a lane then does fetch are the guarded scratch's, as before.
    // The offsets are made opaque: hipcc otherwise re-derives them from the lane id inside the step loops.
    uint32_t doff[2][NDMA], coff[4];
    int yb[2];                                         // a pass's first staged row, clamped
    {
        int l = lane;
        asm volatile("" : "+v"(l));
#pragma unroll
        for (int ps = 0; ps < 2; ps++) {
            const int dylo = ps == 0 ? -RAD : 1;
            yb[ps] = min(max(Y0 + dylo, 0), g.ny - 1);
#pragma unroll
            for (int i = 0; i < NDMA; i++) {
                const unsigned p = 64u * i + (unsigned)l;
                const unsigned r0 = (p * (65536u / PCH + 1u)) >> 16;          // p / PCH for p < 2^12
                const unsigned r = min(r0, (unsigned)(PROWS - 1));
                const unsigned q = min(p - r0 * PCH, (unsigned)(PCOLS / 8 - 1));
                const int yy = min(max(Y0 + dylo + (int)r, 0), g.ny - 1);
                doff[ps][i] = 2u * ((unsigned)(yy - yb[ps]) * (unsigned)g.nx + 8u * q);
                asm volatile("" : "+v"(doff[ps][i]));
            }
        }
#pragma unroll
        for (int y = 0; y < 4; y++) {
            coff[y] = 2u * ((unsigned)(qy - Y0 + y) * (unsigned)g.nx + (unsigned)qx);
            asm volatile("" : "+v"(coff[y]));
        }
    }
    const char* const vol_b = reinterpret_cast<const char*>(vol);
    u32x2 An[4];
    auto load_cell_plane = [&](int step) {
        const char* cbase = vol_b + 2 * ((long long)(qz + (step & 3)) * (long long)sz + (long long)Y0 * (long long)sy);
#pragma unroll
        for (int y = 0; y < 4; y++) {
            // (opaque again, in the step: hipcc otherwise zero-extends the offset outside the loop, into a register
            // pair, and adds the base to it in 64 bits, where instruction selection no longer sees the scalar-base form)
            uint32_t o = coff[y];
            asm volatile("" : "+v"(o));
            const uint32_t* ap = reinterpret_cast<const uint32_t*>(cbase + (size_t)o);
            An[y] = u32x2{ap[0], ap[1]};
        }
    };

    // The staging buffers as LDS-typed pointers: their accesses are ds_ instructions by type.  (As generic pointers
    // they depend on hipcc tracing each one back to pbuf_all, which it gave up on for `cur` / `nxt` once a pass's
    // steps became a loop of their own: it then failed to select the casts back to LDS.)
    using lds_u32 = __attribute__((address_space(3))) uint32_t;
    auto pbuf = [&](int w, int b) { return (lds_u32*)&pbuf_all[w][b][0]; };
    auto issue_dma = [&](int step, lds_u32* dst) {
        const int z = step & 3, pass = (step >> 2) & 1, dz = (step >> 3) - RAD;
        const int pz = min(max(Z0 + z + dz, 0), g.nz - 1);
        // row yb[pass], column X0 of plane pz
        const int yb0 = yb[0], yb1 = yb[1];
        const char* base = vol_b + 2 * ((long long)pz * (long long)sz +
                                        (long long)(pass ? yb1 : yb0) * (long long)sy + X0);
#pragma unroll
        for (int i = 0; i < NDMA; i++) {
            // (values, not a conditional lvalue: a select of two addresses keeps the arrays out of registers)
            const uint32_t o0 = doff[0][i], o1 = doff[1][i];
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(base + (size_t)(pass ? o1 : o0)),
                (__attribute__((address_space(3))) void*)(dst + 256 * i), 16, 0, 0);
        }
    };

    if (!active) {
        // a wave whose cell layer lies beyond the last one any reference block uses only keeps the
        // workgroup's barrier count: two per exchange round (TileShape16::TILE_BARRIERS, as pass_end below)
        for (int i = 0; i < TS::TILE_BARRIERS; i++) __syncthreads();
        break;
    }
    issue_dma(0, pbuf(cz, 0));
    // the first step's cell plane, used (= waited for by hipcc) here: left pending into the loop, it would make
    // hipcc wait vmcnt(0) at the first use of `An` in every step, behind the DMA of the next plane
    load_cell_plane(0);
    asm volatile("" ::"v"(An[0]), "v"(An[1]), "v"(An[2]), "v"(An[3]));

    int acc[NE][SWIN];
#pragma unroll
    for (int e = 0; e < NE; e++)
#pragma unroll
        for (int d = 0; d < SWIN; d++) acc[e][d] = 0;

    // One step = one staged plane.  The first pass of a dz covers dy = -5..0 (six rows of sums), the
    // second dy = 1..5 (five): the body is instantiated for both counts, so no cycles go into a
    // twelfth, masked dy (1024^3: 117.7 -> 114.6 ms).  The float kernel keeps the single body with
    // a masked row: it already sits at 252 registers and the second instantiation spills (131 ->
    // 158 ms measured).
    auto step_body = [&](auto NEc, const int step) {
        constexpr int NEP = decltype(NEc)::value;                 // dy values of this pass
        const int z = step & 3;
        lds_u32* cur = pbuf(cz, step & 1);
        lds_u32* nxt = pbuf(cz, (step + 1) & 1);

        // The waits of a step.  The window rows are read by inline asm, which hipcc leaves
        // out of its wait counts; so none of its own waits falls between the issue of plane step + 1 and the end
        // of the accumulate block.  With plain window reads it waited vmcnt(0) in front of the first one -- an
        // LDS-DMA is a pending LDS write to it, `cur` or `nxt` alike -- i.e. for the plane it had just requested,
        // and the cell's own plane, loaded and used in the same step, cost a second exposed round trip.
        //   vmcnt(0), here: retires the LDS-DMA of THIS step's plane into `cur`, for wave 0 that of the carried
        //     layer into `lower0`, and the loads of this step's cell plane into `An` -- all issued during
        //     step - 1, an accumulate block ago (before the loop for step 0).
        //   lgkmcnt(0), row loop: retires the asm LDS reads of the next window row (`n0`, `n1`), issued in front
        //     of the current row's arithmetic; the statement names them, so no use of them is placed above it.
        // `nxt` may be overwritten from here on: this wave's reads of it were step - 1's window rows, each waited
        // for (lgkmcnt(0)) before its use, and the neighbours' reads of it as an exchange buffer ended behind
        // step - 1's last barrier.  The z == 3 exchange needs no change: it aliases `cur` and reads the
        // neighbour's `cur` behind its own barriers, with plain LDS accesses, in front of which hipcc (and
        // __syncthreads()) still drains the DMA into `nxt` -- by then it has had the accumulate block to land.
        STAMP(t0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(t1);
        // (no code: names `load_cell_plane` ahead of `An`.  This lambda's captures are laid out in the order of their
        // first use, and the order of hipcc's four register copies of `An` at the loop boundaries follows the layout.)
        (void)load_cell_plane;
        const u32x2 A[4] = {An[0], An[1], An[2], An[3]};
        STAMP(t2);
        if (step + 1 < NSTEP) issue_dma(step + 1, nxt);
        if (lower_carried && z == 2)
            carry_prefetch(carry_rd + (size_t)(step >> 2) * 2 * CARRY_ROUND, (lds_u32*)&lower0[0], lane);
        // the next step's cell plane, behind the DMA: retired with it at the top of the next step
        if (step + 1 < NSTEP) load_cell_plane(step + 1);
        asm volatile("" ::: "memory");
        STAMP(t3);

        {
            const lds_u32* wrow_l = cur + ((4 * cy) * PSTR + 4 * cx) / 2;      // dword index
            const uint32_t wrow_lds = (uint32_t)(uintptr_t)wrow_l;
            // staged columns 0..7 / 8..15 of window row r (32 bytes, 8-byte aligned): two ds_read2_b64
            auto read_row = [&](auto rc, u32x4& lo, u32x4& hi) {
                constexpr int r = decltype(rc)::value;
                constexpr int O = r * (PSTR / 4);                                  // in units of 8 bytes
                static_assert(O + 3 < 256, "ds_read2_b64 offsets are 8 bits");
                // (a copy: hipcc does not capture a variable for a generic lambda that names it in an asm operand only)
                const uint32_t row0 = wrow_lds;
                asm volatile("ds_read2_b64 %0, %2 offset0:%3 offset1:%4\n\t"
                             "ds_read2_b64 %1, %2 offset0:%5 offset1:%6"
                             : "=&v"(lo), "=&v"(hi)
                             : "v"(row0), "n"(O), "n"(O + 1), "n"(O + 2), "n"(O + 3));
            };
            auto await_row = [&](u32x4& lo, u32x4& hi) {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi));
            };
            u32x4 q0, q1;
            read_row(std::integral_constant<int, 0>{}, q0, q1);
            await_row(q0, q1);
            STAMP(t4);
            static_for([&](auto rc) {
                constexpr int rp = decltype(rc)::value;
                u32x4 n0, n1;
                if constexpr (rp + 1 < 3 + NEP) read_row(std::integral_constant<int, rp + 1>{}, n0, n1);
                asm volatile("" ::: "memory");
                // W[i] = staged columns (2 i, 2 i + 1); Wo[i] = columns (2 i + 1, 2 i + 2)
                const uint32_t W[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                uint32_t Wo[7];
#pragma unroll
                for (int i = 0; i < 7; i++) Wo[i] = __builtin_amdgcn_alignbit(W[i + 1], W[i], 16);
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    const int e = rp - y;
                    if (e >= 0 && e < NEP) {
#pragma unroll
                        for (int xp = 0; xp < 2; xp++) {
                            const s16x2 a = __builtin_bit_cast(s16x2, xp ? A[y].y : A[y].x);
#pragma unroll
                            for (int d = 0; d < SWIN; d++) {
                                const int j = 1 + 2 * xp + d;            // staged column of voxel x = 2 xp
                                const uint32_t wp = (j & 1) ? Wo[(j - 1) / 2] : W[j / 2];
                                const s16x2 t = __builtin_elementwise_sub_sat(a, __builtin_bit_cast(s16x2, wp));
                                acc[e][d] = __builtin_amdgcn_sdot2(t, t, acc[e][d], true);
                            }
                        }
                    }
                }
                if constexpr (rp + 1 < 3 + NEP) {
                    await_row(n0, n1);
                    q0 = n0;
                    q1 = n1;
                }
            }, std::make_integer_sequence<int, 3 + NEP>{});
            asm volatile("" ::: "memory");
            STAMP(t5);
            STAMP_ADD(0, t0, t1);
            STAMP_ADD(1, t1, t2);
            STAMP_ADD(2, t3, t4);
            STAMP_ADD(3, t4, t5);
        }
    };
    // The end of a pass, behind the accumulate block of its last step (z == 3): publish the sums, select, carry.
    auto pass_end = [&](auto NEc, const int step) {
        constexpr int NEP = decltype(NEc)::value;
        // Exchange rounds of XROWS dy values, the last one of what is left.  The carry slot of a (dz, pass) -- in
        // global memory and in lower0 alike -- is linear [dy row e][d][64 cells], whatever the rounds: round e0's
        // sums lie at e0 * SWIN * 64 (CARRY_ROUND for the second round of three rows).  So the slot's size, the
        // prefetch of a whole slot and the done[] protocol are the same for every round size.
        // A round has two barriers; TS::rounds(NEP) is also what the idle waves' barrier count is made of.
        constexpr int NR0 = XROWS, NROUND = TS::rounds(NEP);
        static_assert((NROUND - 1) * NR0 < NEP && NROUND * NR0 >= NEP, "the rounds cover the pass's rows, none is empty");
#ifdef EXABM4D_BM_STAMPS
        static_assert(2 * NROUND <= BM_STAMP_BARRIERS, "a stamp slot per barrier");
#endif
        const int dz = (step >> 3) - RAD;
        const int dylo = NEP == NE ? -RAD : 1;
        lds_u32* cur = pbuf(cz, step & 1);
        {
            const bool vz = (rz + dz >= 0) && (rz + dz <= g.nz - BLK);
            lds_u32* mine = cur + lane;
            const lds_u32* up_w = cur + lane;                                      // own cells: the upper layer
            // the lower layer: wave cz - 1's sums; for wave 0 the previous block's top layer
            const lds_u32* lo_w = (cz > 0 ? pbuf(max(cz - 1, 0), step & 1) : (lds_u32*)&lower0[0]) + lane;
            uint32_t* cslot = carry_wr + (size_t)((step >> 2) * 2) * CARRY_ROUND + lane;
            // sum of this cell and its x-neighbour; cell sums are capped at 2^27 so that eight of
            // them cannot wrap (a capped sum is far beyond any admissible distance)
            auto pair_sum = [&](int e, int d) {
                const uint32_t c = min((uint32_t)acc[e][d], 1u << 27);
                const uint32_t right = (uint32_t)__builtin_amdgcn_update_dpp(
                    0, (int)c, 0x101 /* row_shl:1 */, 0xF, 0xF, true);
                return c + right;
            };
#pragma unroll
            for (int e0 = 0; e0 < NEP; e0 += NR0) {         // NROUND rounds
#pragma unroll
                for (int e = e0; e < (e0 + NR0 < NEP ? e0 + NR0 : NEP); e++)
#pragma unroll
                    for (int d = 0; d < SWIN; d++) mine[64 * ((e - e0) * SWIN + d)] = pair_sum(e, d);
                STAMP(b0);
                __syncthreads();
                STAMP(b1);
                if (ref_ok) {
                    // a dy row's block sums first (its 22 LDS reads in flight together), then its
                    // candidates one by one: read-add-compare-branch per candidate exposed an LDS round
                    // trip each, with every wave of the workgroup in this phase at the same time
                    // (114.7 -> 111.7 ms; the same change to the fp32 kernel measured no gain)
#pragma unroll
                    for (int e = e0; e < (e0 + NR0 < NEP ? e0 + NR0 : NEP); e++) {
                        uint32_t Sv[1][SWIN];          // one dy row of sums at a time (registers)
#pragma unroll
                        for (int d = 0; d < SWIN; d++) {
                            const lds_u32* c0 = lo_w + (cz == 0 && e0 ? e0 * SWIN * 64 : 0) + 64 * ((e - e0) * SWIN + d);
                            const lds_u32* c1 = up_w + 64 * ((e - e0) * SWIN + d);
                            Sv[0][d] = (c0[0] + c0[TCX]) + (c1[0] + c1[TCX]);
                        }
                        asm volatile("" ::: "memory");
                        const int dy = dylo + e;
                        {
                            const bool vzy = vz && (ry + dy >= 0) && (ry + dy <= g.ny - BLK);
                            const uint32_t cbase =
                                1u + (uint32_t)(((dz + RAD) * SWIN + (dy + RAD)) * SWIN);
                            const bool self_row = (dz == 0) && (dy == 0);
#pragma unroll
                            for (int d = 0; d < SWIN; d++) {
                                const uint32_t S = Sv[0][d];
                                const uint32_t code = (d == RAD && self_row) ? 0u : cbase + d;
                                const bool valid = vzy && ((xmask >> d) & 1u);
                                list_admit(list, thr, keymax, __float_as_uint((float)S), code, valid);
                            }
                        }
                    }
                }
                STAMP(b2);
                __syncthreads();
                STAMP(b3);
                STAMP_ADD(4, b0, b1);
                STAMP_ADD(5, b1, b2);
                STAMP_ADD(4, b2, b3);
#ifdef EXABM4D_BM_STAMPS
                stb[2 * (e0 / NR0)] += b1 - b0;
                stb[2 * (e0 / NR0) + 1] += b3 - b2;
#endif
                if (carries) {
                    // the top wave's sums are the next block's lowest layer (read there by wave 0 in
                    // this same round, i.e. before this slot is written again)
                    uint32_t* cw = cslot + (size_t)(e0 ? e0 * SWIN * 64 : 0);
#pragma unroll
                    for (int e = e0; e < (e0 + NR0 < NEP ? e0 + NR0 : NEP); e++)
#pragma unroll
                        for (int d = 0; d < SWIN; d++)
                            __hip_atomic_store(cw + 64 * ((e - e0) * SWIN + d), pair_sum(e, d), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
#pragma unroll
            for (int e = 0; e < NE; e++)
#pragma unroll
                for (int d = 0; d < SWIN; d++) acc[e][d] = 0;
        }
    };
    // One loop over dz, in it the four steps of the six-row pass, its end, the four steps of the five-row
    // pass, its end: each accumulate body is a loop of its own, so the two bodies' register assignments meet
    // at a pass boundary, twice per dz, and not in front of every step.
    static_assert(NSTEP == 8 * SWIN, "two passes of four planes per dz");
    // ... and the barriers of all that: what an idle wave counts off above
    static_assert(TS::TILE_BARRIERS == (NSTEP / 8) * 2 * (TS::rounds(NE) + TS::rounds(NE - 1)),
                  "idle and working waves pass the same number of barriers");
#pragma unroll 1
    for (int step0 = 0; step0 < NSTEP; step0 += 8) {
#pragma unroll 1
        for (int step = step0; step < step0 + 4; step++) step_body(std::integral_constant<int, NE>{}, step);
        pass_end(std::integral_constant<int, NE>{}, step0 + 3);
#pragma unroll 1
        for (int step = step0 + 4; step < step0 + 8; step++) step_body(std::integral_constant<int, NE - 1>{}, step);
        pass_end(std::integral_constant<int, NE - 1>{}, step0 + 7);
    }

    if (ref_ok) list_store(keys + ((size_t)((size_t)iz * g.gy + iy) * g.gx + ix) * MAXG, list);
    } while (false);

    if (carry.on) {
        // the tile is finished when the top wave's stores have been acknowledged and wave 0's last prefetch has landed
        STAMP(c0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        STAMP(c1);
        STAMP_ADD(6, c0, c1);
        if (threadIdx.x == 0) __hip_atomic_store(done_col, tz + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#ifdef EXABM4D_BM_STAMPS
    st[7] = stamp() - tk0;
    if (lane == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&g_bm_stamps[i], st[i]);
    if (lane == 0)
        for (int i = 0; i < BM_STAMP_BARRIERS; i++) atomicAdd(&g_bm_barrier_stamps[i][tid >> 6], stb[i]);
#endif
}

#ifdef EXABM4D_BM_STAMPS
extern "C" void exabm4d_debug_bm_stamps(unsigned long long* out, int reset) {
    unsigned long long z[8] = {};
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bm_stamps), sizeof(z));
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bm_stamps), z, sizeof(z));
}
// out[6][12]: cycles in each of the (up to six) barriers of a (dz, pass), per wave index
extern "C" void exabm4d_debug_bm_barrier_stamps(unsigned long long* out, int reset) {
    unsigned long long z[BM_STAMP_BARRIERS][BM_STAMP_WAVES] = {};
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bm_barrier_stamps), sizeof(z));
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bm_barrier_stamps), z, sizeof(z));
}
#endif

// ------------------------------------------------------------------------------------------------
// Generic kernel: one wave per reference block, lanes share the 1331 candidates.  Used for the
// clamped last grid position of an axis whose extent is not 8 (mod 4) (e.g. the 54^3 crops of
// evaluate.py:201), and as an independent cross-check of the tile kernel in the parity tests.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bm_generic_kernel(const float* __restrict__ vol_all,
                                                        VolGeom g, uint32_t keymax,
                                                        uint32_t* __restrict__ keys_all,
                                                        int only_unaligned) {
    __shared__ float rb[BVOX];
    const float* __restrict__ vol = vol_all + (size_t)blockIdx.y * (size_t)g.nvox;
    uint32_t* __restrict__ keys = keys_all + (size_t)blockIdx.y * (size_t)g.nref * MAXG;

    const long long r = blockIdx.x;
    const int ix = (int)(r % g.gx), iy = (int)((r / g.gx) % g.gy),
              iz = (int)(r / ((long long)g.gx * g.gy));
    if (only_unaligned && iz < g.az && iy < g.ay && ix < g.ax) return;
    const int rz = grid_pos(iz, g.az, g.nz), ry = grid_pos(iy, g.ay, g.ny),
              rx = grid_pos(ix, g.ax, g.nx);
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
    const int lane = threadIdx.x;

    for (int i = lane; i < BVOX; i += 64) {
        const int bx = i & 7, by = (i >> 3) & 7, bz = i >> 6;
        rb[i] = vol[(size_t)(rz + bz) * sz + (size_t)(ry + by) * sy + (rx + bx)];
    }
    __syncthreads();

    uint32_t list[MAXG];
#pragma unroll
    for (int k = 0; k < MAXG; k++) list[k] = KEY_EMPTY;

    for (int c = lane; c < NCAND; c += 64) {
        const int dx = c % SWIN - RAD, dy = (c / SWIN) % SWIN - RAD, dz = c / (SWIN * SWIN) - RAD;
        const int pz = rz + dz, py = ry + dy, px = rx + dx;
        const bool valid = pz >= 0 && pz <= g.nz - BLK && py >= 0 && py <= g.ny - BLK && px >= 0 &&
                           px <= g.nx - BLK;
        uint32_t key = KEY_EMPTY;
        if (valid) {
            const float* __restrict__ b = vol + (size_t)pz * sz + (size_t)py * sy + px;
            float cell[8];
#pragma unroll 1
            for (int kc = 0; kc < 8; kc++) {
                const int kz = kc >> 2, ky = (kc >> 1) & 1, kx = kc & 1;
                float acc = 0.0f;
#pragma unroll 1
                for (int z = 0; z < 4; z++)
#pragma unroll
                    for (int y = 0; y < 4; y++) {
                        const int bz = 4 * kz + z, by = 4 * ky + y;
                        const float* bp = b + (size_t)bz * sz + (size_t)by * sy + 4 * kx;
                        const float* ap = rb + (bz * 8 + by) * 8 + 4 * kx;
#pragma unroll
                        for (int x = 0; x < 4; x++) {
                            const float t = ap[x] - bp[x];
                            acc = fmaf(t, t, acc);
                        }
                    }
                cell[kc] = acc;
            }
            const float lo = (cell[0] + cell[1]) + (cell[2] + cell[3]);
            const float hi = (cell[4] + cell[5]) + (cell[6] + cell[7]);
            const float S = lo + hi;
            key = (__float_as_uint(S) & KEY_DMASK) | disp_code(dz, dy, dx);
            if (key >= keymax) key = KEY_EMPTY;
        }
        list_insert(list, key);
    }

    // 64 sorted lists -> global top 16: repeatedly take the wave-wide minimum head.
    uint32_t* out = keys + (size_t)r * MAXG;
    for (int k = 0; k < MAXG; k++) {
        uint32_t m = list[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off));
        if (list[0] == m && m != KEY_EMPTY) {
#pragma unroll
            for (int i = 0; i < MAXG - 1; i++) list[i] = list[i + 1];
            list[MAXG - 1] = KEY_EMPTY;
        }
        if (lane == 0) out[k] = (k == 0 && m == KEY_EMPTY) ? 0u : m;      // never empty
    }
}

// ------------------------------------------------------------------------------------------------
// host launchers (called from exabm4d_api.cpp)
// ------------------------------------------------------------------------------------------------
// Workgroup order: 0 = every XCD walks its own contiguous range of tiles (so the XCDs sit in different z
// slabs of a large volume); 1 = all XCDs inside one slab of ty x tx tiles at a time (worth it once a slab
// has a few tiles per CU), raster order inside the slab; n >= 2 = the same, the slab walked in strips of n
// tile rows, column-major inside a strip: the 32 tiles an XCD works on together then form a 2-D patch
// instead of one long row of tiles, a smaller set of cache lines (measured at 1024^3 on a noisy volume: fp32
// kernel 109.4 -> 107.5 ms with strips of 2, 108.7 with 3, 110.0 with 4; the integer kernel and the fp32 kernel
// on the pipeline's smooth basic estimate are indifferent -- DESIGN.md 5.1d).
// (BmOpts::xcd_mode, default 2; BmOpts::carry: 0 = off (tiles advance by seven cell layers), 1 = on wherever it
// saves a tile per column, 2 = on whenever a column has two tiles (tests).  Per context since round 4.)

// Tile shape: fewer (y, x) tiles = fewer idle cell lanes (64^3 patches: 5 flat tiles against 9 cubes)
using Cube = TilePlan<8, 8>;
using Flat = TilePlan<4, 16>;
// Cost of a cell layer in the 12-layer tile (three waves per SIMD, three exchange rounds per pass) over that in
// the 8-layer tile.  Measured with the integer kernel at 1024^3 in slab order with the carry, A/B/A/B on one device,
// twice (profiles/bmlayers/ab.json, "layer_cost_ratio"): 22 tiles x 12 layers in 86.9 ms against 32 x 8 in 91.6-91.8 ms,
// (86.9 / 264) / (91.6 / 256) = 0.920, 0.920, 0.919, 0.919 in the four pairs.  Launches without the carry have not
// been measured at 12 layers and keep 8.
constexpr double BM_LAYER_COST_12_OVER_8 = 0.92;
static bool flat_tiles(const VolGeom& g) {
    auto tiles = [&](int try_, int trx) {
        return (long long)((g.ay + try_ - 1) / try_) * ((g.ax + trx - 1) / trx);
    };
    return tiles(Flat::TRY, Flat::TRX) < tiles(Cube::TRY, Cube::TRX);
}
// The launch block matching chooses for a geometry (host logic only; the float and the integer kernel share
// the tile plan).  Evaluated ONCE per launch by the API layer, which also provides plan.carry_bytes of device
// memory when plan.carry is set.
BmPlan bm_plan(const VolGeom& g, int batch, const BmOpts& opt) {
    BmPlan p = {};
    if (g.az <= 0 || g.ay <= 0 || g.ax <= 0) return p;
    p.flat = flat_tiles(g) ? 1 : 0;
    const int try_ = p.flat ? Flat::TRY : Cube::TRY, trx = p.flat ? Flat::TRX : Cube::TRX;
    p.ty = (g.ay + try_ - 1) / try_;
    p.tx = (g.ax + trx - 1) / trx;
    const long long cols = (long long)p.ty * p.tx * batch;          // columns of tiles: (batch element, ty, tx)
    // tiles of a column: of `l` cell layers without the carry (l - 1 reference layers each) and with it
    auto tz7_of = [&](int l) { return (g.az + l - 2) / (l - 1); };
    auto tz8_of = [&](int l) { return g.az / l + 1; };
    const bool slab = opt.xcd_mode != 0 && cols >= 512;
    // Cell layers per tile of the integer kernel (bm_layers).  Automatic: 12 for the cube shape
    // where the launch is in slab order with the carry on -- the large volumes -- and the 12-layer tiles of a column
    // cost no more than its 8-layer tiles: a column's time is its tiles x layers x the geometry's cost per layer,
    // and a column's last tile counts in full whatever part of it is idle.  BM_LAYER_COST_12_OVER_8 is that cost
    // ratio as measured (see its comment).  Patches, small volumes and launches without the carry keep 8.
    // The carry pays where it saves a tile per column (a 64^3 patch: 15 reference layers = 3 tiles without,
    // 2 with) AND a slab is a couple of rounds of the 256 CUs: a tile waits for the tile below it, and when
    // both are resident together the upper one only spins on a CU (a single small volume gains nothing).
    // 744 KB per column (+ done[columns] + the ticket counter): beyond 16 GB the launch goes without
    const size_t need = 2 * (size_t)cols * CARRY_TILE * sizeof(uint32_t) + ((size_t)cols + 64) * sizeof(int);
    const bool fits = need <= ((size_t)16 << 30);
    auto worth_of = [&](int l) { return tz8_of(l) >= 2 && tz8_of(l) < tz7_of(l) && slab; };
    int layers = TCZ;
    if (opt.layers == 12 && !p.flat) layers = 12;
    if (opt.layers == 0 && !p.flat && opt.carry != 0 && fits && worth_of(TCZ) && worth_of(12) &&
        tz8_of(12) * 12 * BM_LAYER_COST_12_OVER_8 <= tz8_of(TCZ) * TCZ)
        layers = 12;
    p.layers = layers;
    const int tz7 = tz7_of(layers), tz8 = tz8_of(layers);
    const bool worth = worth_of(layers);
    p.carry = (opt.carry != 0 && (worth || (opt.carry == 2 && tz8 >= 2)) && fits) ? 1 : 0;
    p.carry_bytes = p.carry ? need : 0;
    p.tz = p.carry ? tz8 : tz7;
    // ONE plan serves the integer and the fp32 launch of a call.  The carry and the slab order are decided from the
    // integer kernel's tile counts and hold for the fp32 kernel too, which launches tz_f32 slabs of TCZ layers: a
    // FORCED bm_layers = 12 can therefore change the fp32 launch's carry and order as well (correct either way: the
    // carry on means az >= 12, two 8-layer tiles at least; a one-tile column with the carry on carries nothing), and
    // a one-slab 12-layer launch goes in slab order where its 8-layer form has two slabs.  The automatic rule asks
    // for worth_of(8) AND worth_of(12): it changes neither for any launch.
    p.tz_f32 = p.carry ? tz8_of(TCZ) : tz7_of(TCZ);
    p.xq = (p.carry || (slab && (p.tz >= 2 || p.tz_f32 >= 2))) ? (int)((cols + 7) / 8) : 0;
    p.strip = (opt.xcd_mode >= 2 && p.xq) ? opt.xcd_mode : 0;
    p.fault = opt.carry_fault;
    return p;
}

hipError_t launch_blockmatch(const float* vol, const VolGeom& g, int batch, uint32_t keymax,
                             uint32_t* keys, hipStream_t stream, int force_generic, int guarded,
                             const uint16_t* vol16, const BmPlan& p, void* carry_mem, unsigned* status) {
    // vol16 != nullptr: the volume's uint16 counts XOR 0x8000 in guarded scratch; the caller has
    // checked that the integer kernel gives the float kernel's tables (keymax <= 2^24, nx even)
    // carry_mem: p.carry_bytes of device memory when p.carry; status: the context's host-visible status word
    if (p.carry && (!carry_mem || !status)) return hipErrorInvalidValue;
    if (!force_generic && g.az > 0 && g.ay > 0 && g.ax > 0) {
        Carry carry;
        carry.strip = p.strip;
        carry.on = p.carry;
        carry.buf = static_cast<uint32_t*>(carry_mem);
        const size_t cols = (size_t)p.ty * p.tx * (size_t)batch;
        carry.done = p.carry ? reinterpret_cast<int*>(carry.buf + 2 * cols * CARRY_TILE) : nullptr;
        carry.ticket = p.carry ? carry.done + cols : nullptr;
        carry.status = status;
        carry.fault = p.fault;
        if (p.carry) {      // done[columns] and the eight ticket counters behind it
            hipError_t e = hipMemsetAsync(carry.done, 0, (cols + 8) * sizeof(int), stream);
            if (e != hipSuccess) return e;
        }
        // the integer kernel's lanes address a staged plane by 32-bit byte offsets from its first row
        if (vol16 &&
            ((unsigned long long)Cube::PROWS * (unsigned long long)g.nx + 80ull) * 2ull >= (1ull << 32))
            return hipErrorInvalidValue;
        if (p.layers != TCZ && (p.layers != 12 || p.flat)) return hipErrorInvalidValue;
        const int tz = vol16 ? p.tz : p.tz_f32;       // the fp32 kernel's tiles have TCZ layers whatever the plan's
        const dim3 grid((unsigned)(p.xq ? 8 * p.xq * tz : tz * p.ty * p.tx), (unsigned)(p.xq ? 1 : batch));
        auto launch = [&](auto plan) {          // the kernel for the volume's type, in the plan's tile shape
            using Shape16 = TileShape16<decltype(plan)::TCY, decltype(plan)::TCX>;
            using Shape = TileShape<decltype(plan)::TCY, decltype(plan)::TCX>;
            if (vol16)
                hipLaunchKernelGGL(bm_tile16_kernel<Shape16>, grid, dim3(64 * Shape16::LAYERS), 0, stream, vol16, g,
                                   keymax, keys, p.ty, p.tx, p.xq, batch, carry);
            else
                hipLaunchKernelGGL(bm_tile_kernel<Shape>, grid, dim3(512), 0, stream, vol, g, keymax, keys, p.ty,
                                   p.tx, guarded, p.xq, batch, carry);
        };
        if (vol16 && p.layers == 12) {          // the cube's 12-layer tile, three waves per SIMD
            using Shape12 = TileShape16<Cube::TCY, Cube::TCX, 12>;
            hipLaunchKernelGGL(bm_tile16_kernel<Shape12>, grid, dim3(64 * Shape12::LAYERS), 0, stream, vol16, g, keymax,
                               keys, p.ty, p.tx, p.xq, batch, carry);
        } else
        if (p.flat)
            launch(Flat{});
        else
            launch(Cube{});
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const bool unaligned = g.gz != g.az || g.gy != g.ay || g.gx != g.ax;
    if (force_generic || unaligned) {
        dim3 grid((unsigned)g.nref, (unsigned)batch);
        hipLaunchKernelGGL(bm_generic_kernel, grid, dim3(64), 0, stream, vol, g, keymax, keys,
                           force_generic ? 0 : 1);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace exabm4d
