"""The reductions of metrics_kernels.hip against exact references (tests/stream_pyref.py, numpy, math.fsum):
masked error statistics, min / max, the int32 symbol and fp64-key histograms, SSIM; and what a NaN in a
prediction does to the metrics built on them."""
import math

import numpy as np
import pytest

import stream_pyref as P
from oracle import host_oracle as H
from util import GuardedView

from aind_exaspim_image_compression.machine_learning import metrics as M
from aind_exaspim_image_compression.utils import img_util as IU
from aind_exaspim_image_compression.utils import order_stats as OS

pytestmark = pytest.mark.gpu
DTYPES = [np.uint16, np.float32, np.float64]
STAT_NS = [1, 255, 256, 257, 8192 * 256 + 3]        # the last: beyond 8192 workgroups of 256 lanes, the loop wraps
U = 2.0 ** -53


def sum_bound(n):
    """|computed - exact| / exact of ANY summation order of n non-negative doubles (Higham, Accuracy and
    Stability of Numerical Algorithms, eq. 4.4): needs no measurement; one dropped or doubled element of n
    similar ones is an error of about 1 / n, far outside."""
    g = (n - 1) * U
    return g / (1.0 - g)


def values(dtype, n, seed, integer):
    rng = np.random.default_rng(seed)
    if dtype == np.uint16 or integer:
        v = rng.integers(0, 4000, n)
        v[rng.integers(0, n)] = 65535
        return v.astype(dtype)
    v = rng.normal(300.0, 200.0, n)
    v[rng.integers(0, n)] = 70000.123
    return v.astype(dtype)          # float32: 24 random mantissa bits; float64: 53


def thresholds(pred):
    """+inf; a value equal to some pred[i] (the comparison is strict: that voxel does not count); a value
    strictly between two neighbouring values of pred."""
    p = np.unique(pred.astype(np.float64))
    mid = p[p.size // 2]
    between = (p[p.size // 2 - 1] + mid) / 2 if p.size > 1 else mid - 0.5
    return [np.inf, float(mid), float(between)]


@pytest.mark.parametrize("n", STAT_NS)
@pytest.mark.parametrize("rdt", DTYPES)
@pytest.mark.parametrize("pdt", DTYPES)
def test_masked_error_stats(ctx, pdt, rdt, n):
    """All nine dtype pairs, mask NULL / all zero / all one / random, three thresholds, every base pointer one
    element past 16-byte alignment.  Integer-valued inputs: all seven columns EQUAL numpy's integers.  Float
    inputs: the counts and the three maxima equal; each sum within sum_bound(n) of math.fsum."""
    rng = np.random.default_rng(n)
    masks = {"null": None, "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8),
             "random": (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)}
    kinds = [True] if pdt == np.uint16 and rdt == np.uint16 else [True, False]
    for integer in kinds:
        pred, ref = values(pdt, n, n + 1, integer), values(rdt, n, n + 2, integer)
        gp, gr = GuardedView(ctx, pdt, n, 1, pred), GuardedView(ctx, rdt, n, 1, ref)
        p64, r64 = pred.astype(np.float64), ref.astype(np.float64)
        err = np.abs(p64 - r64)
        all_sum = float(err.astype(np.int64).sum()) if integer else math.fsum(err)
        try:
            for mname, mask in masks.items():
                gm = GuardedView(ctx, np.uint8, n, 1, mask) if mask is not None else None
                fg = np.zeros(n, bool) if mask is None else mask != 0
                if not fg.any() or fg.all():
                    sums = [all_sum, 0.0] if fg.all() else [0.0, all_sum]
                elif integer:
                    sums = [float(err[fg].astype(np.int64).sum()), float(err[~fg].astype(np.int64).sum())]
                else:
                    sums = [math.fsum(err[fg]), math.fsum(err[~fg])]
                try:
                    for thr in thresholds(pred):
                        got = ctx.masked_error_stats(gp.ptr, pdt, gr.ptr, rdt, gm.ptr if gm else None, n, thr)
                        what = f"{np.dtype(pdt)}/{np.dtype(rdt)} n={n} mask={mname} thr={thr} integer={integer}"
                        want = [float(fg.sum()), float(np.count_nonzero(p64[~fg] > thr)), p64.max(), r64.max(),
                                err.max()]
                        np.testing.assert_array_equal(got[2:], want, err_msg=what)
                        for c in (0, 1):
                            if integer:
                                assert got[c] == sums[c], what
                            else:
                                assert abs(got[c] - sums[c]) <= sum_bound(n) * sums[c], (what, c, got[c], sums[c])
                finally:
                    if gm:
                        gm.free()
        finally:
            gp.free()
            gr.free()


@pytest.mark.parametrize("n", STAT_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_minmax(ctx, dtype, n):
    rng = np.random.default_rng(n)
    f = np.finfo(dtype) if dtype != np.uint16 else None
    cases = {"positive only": rng.uniform(3.0, 4000.0, n)}
    if dtype != np.uint16:
        cases["negative only"] = -rng.uniform(3.0, 4000.0, n)          # max must leave its -inf seed behind
        cases["zeros of both signs"] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        cases["infinities"] = np.where(rng.random(n) < 0.1, np.inf, rng.normal(0, 1, n))
        cases["minus infinity"] = np.where(rng.random(n) < 0.1, -np.inf, rng.normal(0, 1, n))
        cases["widest finite"] = rng.choice([f.max, -f.max, f.tiny, -f.tiny, 1.0], n)
    if dtype == np.float64:
        cases["beyond float32"] = rng.choice([1e300, -1e300, 1e-300, 3.0000000000000004], n)
    for name, v in cases.items():
        x = v.astype(dtype)
        for where in (0, n - 1, n // 2):               # the extremes at the ends and in the middle
            y = x.copy()
            if name in ("positive only", "negative only"):
                y[where] = dtype(x.max() + 1) if dtype != np.uint16 else 65535
                y[n - 1 - where] = dtype(x.min() - 1) if dtype != np.uint16 else 0
            for k in (0, 1):
                g = GuardedView(ctx, dtype, n, k, y)
                try:
                    got = ctx.minmax(g.ptr, dtype, n)
                finally:
                    g.free()
                assert got == (float(y.min()), float(y.max())), (name, np.dtype(dtype), n, where, k)


# ---- NaN / inf in predictions -------------------------------------------------------------------------
def test_nan_in_a_maximum_column_is_nan(ctx):
    """np.max returns NaN when an element is NaN; fmax alone drops it.  Wherever the NaN sits (first or last
    lane of a workgroup, another workgroup), the maximum of its operand and of |p - r| are NaN, the other
    maximum is not; min / max both are."""
    n = 8192 * 256 + 3
    rng = np.random.default_rng(0)
    base = rng.normal(100, 20, n).astype(np.float32)
    ref = rng.normal(100, 20, n).astype(np.float32)
    gr = GuardedView(ctx, np.float32, n, 0, ref)
    try:
        for at in (0, 255, 256, 70001, n - 1):
            pred = base.copy()
            pred[at] = np.nan
            gp = GuardedView(ctx, np.float32, n, 0, pred)
            try:
                out = ctx.masked_error_stats(gp.ptr, np.float32, gr.ptr, np.float32, None, n)
                assert np.isnan(out[4]) and np.isnan(out[6]) and np.isnan(out[1]), (at, out)
                assert out[5] == float(ref.max()) and out[0] == 0.0 and out[2] == 0.0, (at, out)
                out = ctx.masked_error_stats(gr.ptr, np.float32, gp.ptr, np.float32, None, n)
                assert np.isnan(out[5]) and np.isnan(out[6]) and out[4] == float(ref.max()), (at, out)
                lo, hi = ctx.minmax(gp.ptr, np.float32, n)
                assert np.isnan(lo) and np.isnan(hi), (at, lo, hi)
            finally:
                gp.free()
    finally:
        gr.free()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_metrics_of_a_diverged_prediction_equal_numpys(dtype, bad):
    """A prediction holding a NaN or an infinity (a diverged network) through the metric functions against the
    host oracle's numpy versions: NaN where numpy says NaN."""
    from util import metric_inputs
    _, pf, raw, target, fg = metric_inputs(4)
    for where in ((12, 10, 14), (30, 30, 30)):            # one foreground voxel, one background voxel
        assert bool(fg[where]) == (where == (12, 10, 14))
        pred = pf.astype(dtype)
        pred[where] = bad
        with np.errstate(invalid="ignore"):
            np.testing.assert_equal(M.evaluate_example(pred, raw, target, fg), H.evaluate_example(pred, raw, target, fg))
            np.testing.assert_equal(M.mip_max_error(pred, raw), H.mip_max_error(pred, raw))
            np.testing.assert_equal(IU.compute_lmax(pred, raw), H.compute_lmax(pred, raw))
            np.testing.assert_equal(IU.compute_mae(pred, raw), H.compute_mae(pred, raw))
            np.testing.assert_equal(IU.compute_lmax(raw, pred), H.compute_lmax(raw, pred))


# ---- int32 symbol histogram ----------------------------------------------------------------------------
SYM_CHUNK = 28672           # indices one workgroup takes per round: 1024 lanes * 7 vectors * 4
SYM_EDGES = np.array([0, 1, -1, 32766, 32767, 32768, 32769, -32766, -32767, -32768, -32769, 2 ** 31 - 1, -2 ** 31],
                     dtype=np.int32)


def symbol_indices(n, seed):
    rng = np.random.default_rng(seed)
    v = np.rint(rng.laplace(0, 3000, n)).astype(np.int64)
    far = rng.random(n) < 0.02
    v[far] = rng.integers(-2 ** 31, 2 ** 31, int(far.sum()))
    v = v.astype(np.int32)
    k = min(n, SYM_EDGES.size)
    v[:k] = SYM_EDGES[:k]
    if n >= 2 * SYM_EDGES.size:
        v[-SYM_EDGES.size:] = SYM_EDGES[::-1]
    return v


@pytest.mark.parametrize("n", [1, 3, 4, 5, SYM_CHUNK - 1, SYM_CHUNK, SYM_CHUNK + 1, 300_007, 1024 * SYM_CHUNK + 5])
def test_i32_symbol_histogram(ctx, n):
    """Against np.bincount of the restated symbol: the escape boundary at +-32767 / +-32768 and the int32 ends
    at both ends of the array (vector body and scalar tail), n around the four-index vector and the
    workgroup's chunk, more chunks than workgroups; base pointer 16-byte aligned and 4 bytes past it."""
    v = symbol_indices(n, n)
    want = P.i32_symbol_histogram(v)
    for k in ((0, 1) if n <= 300_007 else (0,)):
        g = GuardedView(ctx, np.int32, n, k, v)
        try:
            np.testing.assert_array_equal(ctx.i32_symbol_histogram(g.ptr, n), want, err_msg=f"n={n} offset={k}")
        finally:
            g.free()


def test_i32_symbol_histogram_one_symbol_for_a_whole_chunk(ctx):
    """One symbol repeated over whole chunks: the packed 16-bit LDS counters are flushed before they carry."""
    n = 3 * SYM_CHUNK + 2
    for value in (0, 5, -32767, 32767, 40000):
        v = np.full(n, value, np.int32)
        v[SYM_CHUNK] = 6                                      # the neighbour in the same LDS dword
        g = GuardedView(ctx, np.int32, n, 0, v)
        try:
            np.testing.assert_array_equal(ctx.i32_symbol_histogram(g.ptr, n), P.i32_symbol_histogram(v))
        finally:
            g.free()


# ---- fp64-key digit histograms --------------------------------------------------------------------------
def key_sample(dtype, seed=9, n=6007):
    rng = np.random.default_rng(seed)
    if dtype == np.uint16:
        x = rng.integers(0, 5000, n).astype(np.uint16)
        x[:4] = [0, 65535, 1, 32768]
        return x
    f = np.finfo(dtype)
    special = [0.0, -0.0, np.inf, -np.inf, f.max, -f.max, f.tiny, -f.tiny, f.smallest_subnormal,
               -f.smallest_subnormal, f.tiny / 4, -f.tiny / 4, 1.0, -1.0]
    x = rng.normal(100.0, 400.0, n).astype(dtype)
    x[:len(special)] = np.array(special, dtype=dtype)
    x[100:120] = x[50]                                           # ties
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_histogram_every_digit_and_prefix(ctx, dtype):
    x = key_sample(dtype)
    n = x.size
    centers = [None, float(x[50]), float(np.median(x[np.isfinite(x.astype(np.float64))]))]   # x[50]: an element (twenty times)
    for k in (0, 1):
        g = GuardedView(ctx, dtype, n, k, x)
        try:
            for center in centers:
                keys = P.f64_keys(x, center)
                picks = np.unique(np.concatenate([keys[:16], keys[50:52], [keys.min(), keys.max()],
                                                  np.sort(keys)[[n // 2, n // 3]]]))
                up = {0: ctx.key_histogram(g.ptr, dtype, n, 0, 0, center)}
                np.testing.assert_array_equal(up[0], P.key_digit_histogram(keys, 0), err_msg=f"digit 0 {center}")
                assert int(up[0].sum()) == n
                for digit in (1, 2, 3):
                    for key in picks:
                        prefix = int(key) >> (64 - 16 * digit)
                        got = ctx.key_histogram(g.ptr, dtype, n, digit, prefix, center)
                        what = f"{np.dtype(dtype)} digit {digit} prefix {prefix:#x} center {center} offset {k}"
                        np.testing.assert_array_equal(got, P.key_digit_histogram(keys, digit, prefix), err_msg=what)
                        parent = (ctx.key_histogram(g.ptr, dtype, n, digit - 1, prefix >> 16, center)
                                  if digit > 1 else up[0])
                        assert int(got.sum()) == int(parent[prefix & 0xFFFF]) > 0, what
        finally:
            g.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_radix_selection_returns_every_order_statistic(ctx, dtype):
    """DeviceOrderStats.at(k) for EVERY k of a 4097-element array against np.sort (values and the sign of zero)."""
    rng = np.random.default_rng(12)
    pool = np.unique(key_sample(dtype, seed=13, n=260))
    x = rng.choice(pool, 4097)
    x[:pool.size] = pool
    if dtype != np.uint16:
        x[-4:] = [0.0, -0.0, -0.0, 0.0]
    g = GuardedView(ctx, dtype, x.size, 1, x)
    try:
        st = OS.DeviceOrderStats(ctx, g.ptr, dtype, x.size)
        got = np.array([st.at(k) for k in range(x.size)])
        want = x.astype(np.float64)[np.argsort(P.f64_keys(x), kind="stable")]      # np.sort with -0.0 before +0.0
        np.testing.assert_array_equal(want, np.sort(x.astype(np.float64)))
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(np.signbit(got), np.signbit(want))
    finally:
        g.free()


# ---- SSIM --------------------------------------------------------------------------------------------------
def ssim_gpu(ctx, a, b, window, c1, c2):
    ga, gb = GuardedView(ctx, a.dtype, a.size, 0, a), GuardedView(ctx, b.dtype, b.size, 0, b)
    try:
        return ctx.ssim3d_sum(ga.ptr, gb.ptr, a.dtype, a.shape, window, c1, c2) / a.size
    finally:
        ga.free()
        gb.free()


@pytest.mark.parametrize("shape,window", [((8, 8, 8), 3), ((20, 33, 70), 16), ((37, 18, 129), 7), ((70, 17, 64), 1),
                                          ((16, 100, 65), 32)])
def test_ssim_float32_volumes(ctx, shape, window):
    """The float32 kernel on its own (ssim3D widens float input to float64 before it uploads): benign data,
    running fp64 box sums on both sides, the 1e-9 of the float64 case in test_metrics_gpu.py."""
    rng = np.random.default_rng(sum(shape) + window)
    a = rng.normal(300, 60, shape).astype(np.float32)
    b = (a + rng.normal(0, 25, shape)).astype(np.float32)
    L = float(max(a.max() - a.min(), b.max() - b.min()))
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    assert ssim_gpu(ctx, a, b, window, c1, c2) == pytest.approx(H.ssim3d(a, b, data_range=L, window_size=window), rel=1e-9)


def hostile_volumes(shape, kind):
    rng = np.random.default_rng(sum(shape))
    if kind == "spikes":             # background 1e-3, isolated voxels of 1e6: squares of 1e12 enter and leave the
        a = np.full(shape, 1e-3)     # running sums next to squares of 1e-6
        b = np.full(shape, 1e-3)
        for v, amp in ((a, 1e6), (b, 0.9e6)):
            idx = rng.integers(0, a.size, max(2, a.size // 900))
            v.reshape(-1)[idx] = amp
        b.reshape(-1)[rng.integers(0, a.size, 3)] = 1e6
        return a, b, 1.0             # a caller's data_range of 1: C2 = 9e-4 does not hide what the sums leave behind
    a = np.full(shape, 0.1)          # a constant: every variance cancels to 0 (0.1 is no dyadic fraction)
    return a, a.copy(), 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["spikes", "constant"])
@pytest.mark.parametrize("shape,window", [((12, 20, 70), 7), ((9, 17, 66), 16), ((24, 16, 64), 3)])
def test_ssim_hostile_data_against_direct_window_sums(ctx, shape, window, kind, dtype):
    """Against window sums taken directly from the reflect-padded volume in np.longdouble (no running sums).
    The kernel and scipy's uniform_filter1d run the same add-the-entering, subtract-the-leaving scheme over
    different lengths (a march of up to 64 planes here, whole axes there), so the kernel may deviate from the
    direct value by at most 4 x what scipy (oracle.host_oracle.ssim3d) deviates on the same input.
    Measured scipy deviations (|oracle.host_oracle.ssim3d - direct|, float64 and float32 input alike), in the
    order of the shapes below: spikes 4.4e-07, 9.0e-10, 4.5e-06; constant 3.3e-16, 1.0e-15, 5.6e-16 (float32
    input: 4.4e-16 each).  The test prints both deviations."""
    a, b, L = hostile_volumes(shape, kind)
    a, b = a.astype(dtype), b.astype(dtype)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    direct = P.ssim3d_direct(a, b, window, c1, c2)
    scipy_dev = abs(float(H.ssim3d(a, b, data_range=L, window_size=window)) - direct)
    got = ssim_gpu(ctx, a, b, window, c1, c2)
    print(f"ssim hostile {kind} {np.dtype(dtype)} {shape} w={window}: direct {direct!r} scipy dev {scipy_dev:.3e} "
          f"kernel dev {abs(got - direct):.3e}")
    assert abs(got - direct) <= 4.0 * scipy_dev        # scipy_dev: measured, see the docstring


@pytest.fixture(scope="module")
def long_march_case():
    """70 x 1024 x 1024 uint16: 16 * 64 tiles of 64 x 16 and two z chunks make 2048 workgroups, so the z chunk
    stays at 64 planes (the first chunk marches 64, the second 6).  The host reference once per session, in
    overlapping z slabs so that scipy's float64 temporaries stay small; integer data: every local moment is
    exact whatever the slab."""
    from scipy.ndimage import uniform_filter
    shape, w = (70, 1024, 1024), 16
    rng = np.random.default_rng(70)
    a = np.clip(rng.normal(300, 60, shape), 0, 65535).astype(np.uint16)
    a[35, 512, 512] = 40000
    b = np.clip(a.astype(np.float32) + rng.normal(0, 25, shape).astype(np.float32), 0, 65535).astype(np.uint16)
    L = float(max(int(a.max()) - int(a.min()), int(b.max()) - int(b.min())))
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    total, step = 0.0, 256
    for y0 in range(0, shape[1], step):      # slabs along y with a halo of one window: z and x keep their true ends
        lo, hi = max(0, y0 - w), min(shape[1], y0 + step + w)
        sa, sb = a[:, lo:hi].astype(np.float64), b[:, lo:hi].astype(np.float64)
        box = lambda v: uniform_filter(v, w)[:, y0 - lo:y0 - lo + step]   # noqa: E731
        m1, m2 = box(sa), box(sb)
        v1, v2, v12 = box(sa * sa) - m1 * m1, box(sb * sb) - m2 * m2, box(sa * sb) - m1 * m2
        num = (2 * m1 * m2 + c1) * (2 * v12 + c2)
        den = (m1 * m1 + m2 * m2 + c1) * (v1 + v2 + c2)
        total += float(np.sum(num / (np.maximum(den, 1e-8) + 1e-6)))
    return a, b, w, c1, c2, total / a.size


def test_ssim_long_march_on_a_large_uint16_volume(ctx, long_march_case):
    a, b, w, c1, c2, want = long_march_case
    assert ssim_gpu(ctx, a, b, w, c1, c2) == pytest.approx(want, rel=1e-12)
