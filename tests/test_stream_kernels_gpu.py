"""Every entry point of the elementwise stream family (launch_stream: eight voxels per lane when all
pointers are 16-byte aligned, one per lane for the tail and for unaligned views) bit for bit against
tests/stream_pyref.py, on views into larger buffers.

Each operand lives inside a DeviceBuffer with a guard band on both sides (util.GuardedView); the kernel is
handed ``buf.ptr + guard + k * itemsize``.  Asserted per case: (a) the n outputs equal the reference exactly
(these operations are correctly rounded IEEE steps), (b) every byte around the output view is unchanged,
(c) the inputs are unchanged unless the call aliases them.

n runs over the 8-voxel boundary, the 256-lane workgroup boundary and beyond one grid's worth of vector lanes
(2048 workgroups * 256 lanes * 8 voxels = 4 194 304, where the grid-stride loops wrap).  All five offsets run at
every n up to 2049 -- the values at the ties, the clamp ends and the infinities repeat every 128 voxels, so
those n hold all of them on both paths -- and the large n, which is there for the wrap, runs one."""
import numpy as np
import pytest

import stream_pyref as P
from oracle import host_oracle as H
from test_oracle_golden import TRANSFORM_CFGS
from util import GuardedView

from aind_exaspim_image_compression.machine_learning import transforms as T

pytestmark = pytest.mark.gpu
F32 = np.float32

BIG = 2 * 4_194_304 + 13
NS = [1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, BIG]
OFFSETS = [0.0, 37.0, -12.5, 36.73, 65536.0]
# element offsets (first input, other inputs, output)
VIEWS = {"aligned": (0, 0, 0), "in+1": (1, 0, 0), "out+1": (0, 0, 1), "all+1": (1, 1, 1), "in+8": (8, 0, 0)}


def offsets_for(n):
    return OFFSETS if n < BIG else [36.73]


def run_views(ctx, inputs, out_dtype, want, call, what, inplace=False):
    """`call(in_ptrs, out_ptr, n)` on every view arrangement; `want`: the n expected outputs."""
    n = want.size
    for name, (k0, k1, ko) in VIEWS.items():
        ins = [GuardedView(ctx, a.dtype, n, k0 if j == 0 else k1, a) for j, a in enumerate(inputs)]
        out = ins[0] if inplace else GuardedView(ctx, out_dtype, n, ko)
        try:
            call([v.ptr for v in ins], out.ptr, n)
            ctx.sync()
            out.check_output(want, f"{what}, {name}")
            for v in ins[1 if inplace else 0:]:
                v.check_untouched(f"{what}, {name}")
        finally:
            for v in ins + ([] if inplace else [out]):
                v.free()
        if inplace and name == "in+1":
            break                      # one pointer: aligned and off by one are all there is


def edge_counts(n, offset, seed):
    """fp32 values x with x + offset at the ties k + 0.5 (even and odd k), just below 0, at 0, around both
    clamp ends, far outside, and infinite -- 64 of them, repeated, with random counts in between."""
    targets = np.array([0.5, 1.5, 2.5, 3.5, 6.5, 7.5, 100.5, 101.5, 1000.5, 1001.5, 32766.5, 32767.5, 32768.5,
                        65532.5, 65533.5, 65534.5, 65535.5, 65535.0, 65534.0, 65535.25, 65534.75, 65536.0, 0.0,
                        -0.0, -0.25, -0.5, -0.75, -1e-3, -1.0, -70000.0, 70000.0, 1e30, -1e30, np.inf, -np.inf,
                        0.25, 0.75, 0.49999997, 0.50000006, 1.4999999, 1.5000001, 2.4999998, 2.5000002],
                       dtype=np.float64)
    off = np.float64(F32(offset))
    with np.errstate(over="ignore", invalid="ignore"):
        block = np.concatenate([(targets - off).astype(F32), targets.astype(F32)])[:64]
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-200.0, 66000.0, n) - off).astype(F32)
    reps = -(-n // 128)
    idx = (np.arange(reps)[:, None] * 128 + np.arange(64)[None, :]).reshape(-1)
    idx = idx[idx < n]
    x[idx] = np.resize(block, reps * 64)[:idx.size]
    return x


def quotient_operands(n, offset, seed):
    """(num, den) whose fp32 quotients are edge_counts: den a power of two (exact quotients: ties k + 0.5 from
    odd numerators over 2), tiny den with finite num for the infinite ones, random den elsewhere."""
    q = edge_counts(n, offset, seed)
    rng = np.random.default_rng(seed + 1)
    den = np.exp2(rng.integers(-3, 4, n)).astype(F32)
    rnd = rng.random(n) < 0.3
    den[rnd] = rng.uniform(0.3, 9.0, int(rnd.sum())).astype(F32)
    inf = np.isinf(q)
    den[inf] = F32(1e-30)
    with np.errstate(over="ignore", invalid="ignore"):
        num = np.where(inf, np.sign(q) * F32(1e30), q * den).astype(F32)
    return num, den


# ---- counts_from_u16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_counts_from_u16(ctx, n):
    """All 65536 inputs once n allows, every count at its place modulo 65536 before."""
    v = (np.arange(n, dtype=np.int64) * 40503 % 65536).astype(np.uint16)     # a permutation of the counts
    v[:min(n, 4)] = np.array([0, 65535, 1, 32768], np.uint16)[:min(n, 4)]
    if n >= 65536:
        assert np.unique(v).size == 65536
    for off in offsets_for(n):
        run_views(ctx, [v], F32, P.counts_from_u16(v, off),
                  lambda i, o, m, off=off: ctx.counts_from_u16(i[0], o, m, off), f"counts_from_u16 n={n} offset={off}")


# ---- round_counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_round_counts(ctx, n):
    for off in offsets_for(n):
        x = edge_counts(n, off, n)
        want = P.round_counts(x, off)
        call = lambda i, o, m, off=off: ctx.round_counts(i[0], o, m, off)   # noqa: E731
        run_views(ctx, [x], F32, want, call, f"round_counts n={n} offset={off}")
        run_views(ctx, [x], F32, want, call, f"round_counts in place n={n} offset={off}", inplace=True)


# ---- normalize_u16 / normalize -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_normalize_u16(ctx, n):
    for off in offsets_for(n):
        num, den = quotient_operands(n, off, n)
        run_views(ctx, [num, den], np.uint16, P.normalize_u16(num, den, off),
                  lambda i, o, m, off=off: ctx.normalize_u16(i[0], i[1], o, m, off),
                  f"normalize_u16 n={n} offset={off}")


@pytest.mark.parametrize("n", NS)
def test_normalize(ctx, n):
    num, den = quotient_operands(n, 0.0, n + 7)
    for clip in (None, (0.0, 65535.0), (-12.5, 1000.25)):
        run_views(ctx, [num, den], F32, P.normalize(num, den, clip),
                  lambda i, o, m, clip=clip: ctx.normalize(i[0], i[1], o, m, clip=clip), f"normalize n={n} clip={clip}")


# ---- tile_finalize -----------------------------------------------------------------------------------------
def finalize_operands(n, seed):
    """accum_pred / accum_wgt as the stitching leaves them: weights 0 (the untouched rim), 1, 2, 4, 8 and odd
    counts; predictions from below the transforms' range to above it, and huge ones over a zero weight
    (quotients of +-1e38: beyond every clamp)."""
    rng = np.random.default_rng(seed)
    wgt = rng.choice(np.array([0, 1, 2, 3, 4, 5, 8], F32), n)
    y = rng.uniform(-0.2, 1.2, n).astype(F32)
    acc = (y * wgt).astype(F32)
    acc[wgt == 0] = rng.choice(np.array([0.0, 0.0, 1e30, -1e30, 1e-9], F32), int((wgt == 0).sum()))
    return acc, wgt


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(TRANSFORM_CFGS))
def test_tile_finalize(ctx, name, n):
    cfg = TRANSFORM_CFGS[name]
    tf = T.build_transform(cfg).native_struct()
    acc, wgt = finalize_operands(n, n)
    want = P.tile_finalize(cfg, acc, wgt)
    run_views(ctx, [acc, wgt], np.uint16, want, lambda i, o, m: ctx.tile_finalize(tf, i[0], i[1], o, m),
              f"tile_finalize {name} n={n}")


# ---- transforms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(TRANSFORM_CFGS))
def test_transforms_on_views(ctx, name, n):
    """forward uint16 (direct below 2^20 voxels; the 65536-entry table from there on for the asinh kinds, here
    on unaligned views too), forward fp32, inverse to uint16 and to fp32."""
    cfg = TRANSFORM_CFGS[name]
    tf, o = T.build_transform(cfg).native_struct(), H.TransformOracle(cfg)
    u16 = (np.arange(n, dtype=np.int64) * 40503 % 65536).astype(np.uint16)
    f32_in = np.linspace(-50.0, 70000.0, max(n, 2), dtype=F32)[:n]
    grid = np.linspace(-0.2, 1.2, max(n, 2), dtype=F32)[:n]
    run_views(ctx, [u16], F32, o.forward(u16), lambda i, out, m: ctx.transform_forward(tf, i[0], out, m, True),
              f"forward u16 {name} n={n}")
    run_views(ctx, [f32_in], F32, o.forward(f32_in), lambda i, out, m: ctx.transform_forward(tf, i[0], out, m, False),
              f"forward f32 {name} n={n}")
    run_views(ctx, [grid], np.uint16, o.inverse(grid), lambda i, out, m: ctx.transform_inverse(tf, i[0], out, m),
              f"inverse u16 {name} n={n}")
    run_views(ctx, [grid], F32, o.inverse_float(grid),
              lambda i, out, m: ctx.transform_inverse(tf, i[0], out, m, quantise=False), f"inverse f32 {name} n={n}")


def test_table_path_equals_direct_evaluation_on_an_unaligned_view(ctx):
    """The same 2^20 + 13 counts at an odd element offset through the table (one call) and directly (two calls
    below 2^20 voxels): identical bits."""
    cfg = TRANSFORM_CFGS["offset37_asinh_s32"]
    tf = T.build_transform(cfg).native_struct()
    n = (1 << 20) + 13
    v = np.random.default_rng(0).integers(0, 65536, n).astype(np.uint16)
    src = GuardedView(ctx, np.uint16, n, 1, v)
    a, b = GuardedView(ctx, F32, n, 1), GuardedView(ctx, F32, n, 3)
    try:
        ctx.transform_forward(tf, src.ptr, a.ptr, n, True)
        half = n // 2
        ctx.transform_forward(tf, src.ptr, b.ptr, half, True)
        ctx.transform_forward(tf, src.ptr + 2 * half, b.ptr + 4 * half, n - half, True)
        ctx.sync()
        want = H.TransformOracle(cfg).forward(v)
        a.check_output(want, "table")
        b.check_output(want, "direct")
    finally:
        for g in (src, a, b):
            g.free()


# ---- NaN ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_nan_quantises_to_count_zero(ctx, k):
    """include/exabm4d.h: the clamp is fminf(fmaxf(x, 0), 65535) and fmaxf drops a NaN, so a NaN becomes count 0
    on both paths (np.clip would keep it, and a cast of NaN has no defined value: hence its own test)."""
    n = 19
    x = np.linspace(5.0, 23.0, n).astype(F32)
    nan_at = [0, 7, 8, 18]
    x[nan_at] = np.nan
    ones = np.ones(n, F32)
    clean = np.where(np.isnan(x), F32(0), x)
    tf = T.build_transform(TRANSFORM_CFGS["linear_35_1000_8"]).native_struct()

    def run(inputs, out_dtype, call):
        ins = [GuardedView(ctx, F32, n, k, a) for a in inputs]
        out = GuardedView(ctx, out_dtype, n, k)
        try:
            call([v.ptr for v in ins], out.ptr)
            ctx.sync()
            return out.buf.download(out.host.shape, np.uint8)[out.lo:out.hi].view(out_dtype)
        finally:
            for v in ins + [out]:
                v.free()

    got = run([x, ones], np.uint16, lambda i, o: ctx.normalize_u16(i[0], i[1], o, n, 37.0))
    want = P.normalize_u16(clean, ones, 37.0)
    want[nan_at] = 0
    np.testing.assert_array_equal(got, want)
    got = run([x], F32, lambda i, o: ctx.round_counts(i[0], o, n, 37.0))
    want = P.round_counts(clean, 37.0)
    want[nan_at] = F32(-37.0)
    np.testing.assert_array_equal(got, want)
    got = run([x, ones], np.uint16, lambda i, o: ctx.tile_finalize(tf, i[0], i[1], o, n))
    want = P.tile_finalize(TRANSFORM_CFGS["linear_35_1000_8"], clean, ones)
    want[nan_at] = 0
    np.testing.assert_array_equal(got, want)
    got = run([x, ones], F32, lambda i, o: ctx.normalize(i[0], i[1], o, n, clip=(2.0, 20.0)))
    want = P.normalize(clean, ones, (2.0, 20.0))
    want[nan_at] = F32(2.0)
    np.testing.assert_array_equal(got, want)
    got = run([x, ones], F32, lambda i, o: ctx.normalize(i[0], i[1], o, n))
    np.testing.assert_array_equal(got, x)           # no clamp: the NaN stays (assert_array_equal pairs NaNs)
