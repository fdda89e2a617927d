"""The noise table through the C-ABI (exabm4d_noise_table_dev) and the Python surface on it (utils/noise.py,
sigma="auto") against the numpy restatement tests/noise_pyref.py.  The table is integer work and the estimators on
it are the same float64 steps, so everything here is compared for equality."""
import ctypes
import math

import numpy as np
import pytest

import noise_pyref as P
from util import GuardedView, synth_volume

from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression import bm4d as B
from aind_exaspim_image_compression.machine_learning import transforms as T
from aind_exaspim_image_compression.machine_learning.metrics import DeviceImage
from aind_exaspim_image_compression.utils import noise as N

pytestmark = pytest.mark.gpu
SHAPES = [(64, 64, 64), (65, 63, 66), (2, 2, 2), (40, 36, 44), (3, 130, 258)]
SHIFTS = range(7)


def volume(shape, dtype, seed=0):
    """uint16: pedestal + neurites + noise, rounded.  float32: the same before rounding, minus an offset, so that it
    holds fractions and negative counts."""
    if dtype == np.uint16:
        return synth_volume(shape, seed=seed, as_u16=True)[0]
    return synth_volume(shape, seed=seed)[0] - np.float32(30.25)


def device_table(ctx, vol, shift):
    buf = ctx.to_device(vol)
    try:
        return ctx.noise_table(buf, vol.dtype, vol.shape, shift)
    finally:
        buf.free()


def assert_tables_equal(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what}: hist")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: sum_s")
    assert int(got[2]) == int(want[2]), f"{what}: skipped"


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_table_equals_pyref(ctx, shape, dtype):
    vol = volume(shape, dtype, seed=sum(shape))
    buf = ctx.to_device(vol)
    try:
        for shift in SHIFTS:
            got = ctx.noise_table(buf, dtype, shape, shift)
            assert got[0].dtype == np.uint64 and got[0].shape == (P.LEVELS, P.BINS)
            assert_tables_equal(got, P.table(vol, shift), f"{shape} {np.dtype(dtype).name} shift {shift}")
        assert int(got[0].sum()) == (shape[0] // 2) * (shape[1] // 2) * (shape[2] // 2)
    finally:
        buf.free()


@pytest.mark.parametrize("sigma", [800.0, 9000.0])
def test_table_with_wide_noise_equals_pyref(ctx, sigma):
    """Many levels at once (more than the eight a workgroup keeps on chip) and cells beyond the last bin.  Every row
    climbs geometrically from 16 to 40000 counts, so each workgroup meets levels that share a slot."""
    rng = np.random.default_rng(9)
    ramp = 16.0 * 2500.0 ** (np.arange(64) / 63.0)
    vol = to_u16(ramp + rng.normal(0, sigma, (40, 48, 64)))
    hist = P.table(vol, 0)[0]
    assert np.count_nonzero(hist.sum(axis=1)) > 8 and hist[:, -1].sum() > 0
    for dtype in (np.uint16, np.float32):
        for shift in (0, 3, 6):
            v = vol.astype(dtype)
            assert_tables_equal(device_table(ctx, v, shift), P.table(v, shift), f"{dtype} {shift}")


def test_extreme_values_in_one_cell(ctx):
    vol = np.zeros((4, 4, 8), dtype=np.uint16)
    vol[0, 0, 0] = 65535                                   # one bright voxel: s = |d| = 65535
    vol[2:4, 2:4, 2:4] = 65535                             # the largest s, d = 0
    vol[2, 0, 4], vol[2, 1, 5], vol[3, 0, 5], vol[3, 1, 4] = 65535, 65535, 65535, 65535    # |d| = 4 * 65535
    for shift in SHIFTS:
        want = P.table(vol, shift)
        assert_tables_equal(device_table(ctx, vol, shift), want, f"shift {shift}")
        assert_tables_equal(device_table(ctx, vol.astype(np.float32), shift), want, f"fp32, shift {shift}")
    assert want[0][48, 0] == 1 and want[1][48] == 8 * 65535


def test_fp32_negative_counts_nan_and_inf(ctx):
    vol = volume((40, 36, 44), np.float32, seed=5)
    assert (vol < 0).any()
    clean = P.table(vol, 1)
    bad = vol.copy()
    bad[3, 4, 5] = np.nan
    bad[8, 9, 10] = np.inf
    bad[8, 9, 11] = np.inf
    bad[12, 0, 0] = -np.inf
    bad[20, 20, 20] = 3.0e38                               # finite, |d| >= 2^24: the last bin, not skipped
    bad[30, 30, 30], bad[30, 30, 31] = 3.0e38, 3.0e38      # s overflows to inf: skipped
    want = P.table(bad, 1)
    assert want[2] == 4 and want[0].sum() == clean[0].sum() - 4
    got = device_table(ctx, bad, 1)
    assert_tables_equal(got, want)
    keep = vol.copy()                                      # the other cells are not affected
    for z, y, x in ((2, 4, 4), (8, 8, 10), (12, 0, 0), (30, 30, 30)):
        keep[z:z + 2, y:y + 2, x:x + 2] = np.nan
    keep[20, 20, 20] = 3.0e38
    np.testing.assert_array_equal(got[0], P.table(keep, 1)[0])
    assert device_table(ctx, np.full((4, 4, 4), np.nan, np.float32), 0)[2] == 8


@pytest.mark.parametrize("shape", [(64, 64, 64), (40, 36, 44), (65, 63, 66)])
def test_integer_valued_fp32_gives_the_u16_table(ctx, shape):
    vol = volume(shape, np.uint16, seed=11)
    vol[1, 1, 1], vol[0, 0, 0] = 65535, 0
    for shift in (0, 2, 6):
        a = device_table(ctx, vol, shift)
        b = device_table(ctx, vol.astype(np.float32), shift)
        assert_tables_equal(b, a, f"shift {shift}")
        assert a[2] == 0


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape", [(64, 64, 64), (40, 36, 44), (5, 6, 7)])
def test_unaligned_guarded_views(ctx, shape, dtype):
    """Element offsets 0, 1 and 3 from a 16-byte boundary: the same table, and not a byte of the buffer written."""
    vol = volume(shape, dtype, seed=3)
    want = P.table(vol, 1)
    for k in (0, 1, 3):
        g = GuardedView(ctx, dtype, vol.size, k, vol)
        try:
            assert_tables_equal(ctx.noise_table(g.ptr, dtype, shape, 1), want, f"offset {k}")
            g.check_untouched(f"offset {k}")
        finally:
            g.free()


def test_two_launches_and_batches(ctx):
    vol = volume((64, 64, 64), np.uint16, seed=2)
    assert_tables_equal(device_table(ctx, vol, 0), device_table(ctx, vol, 0), "second launch")
    for nz in (16, 15):                                    # even: one launch over the batch; odd: patch by patch
        for dtype in (np.uint16, np.float32):
            batch = np.stack([volume((nz, 18, 24), dtype, seed=s) for s in range(5)])
            want = P.table(batch, 2)
            sep = [P.table(p, 2) for p in batch]
            np.testing.assert_array_equal(want[0], sum(s[0] for s in sep))
            t = N.noise_table(batch, shift=2)
            assert_tables_equal((t.hist, t.sum_s, t.skipped), want, f"batch nz {nz}")
            assert t.shift == 2
            np.testing.assert_array_equal(t.counts, want[0].sum(axis=1))


def test_noise_table_fields_and_resident_inputs(ctx):
    vol = volume((40, 36, 44), np.uint16, seed=8)
    t = N.noise_table(vol)
    hist, sum_s, skipped, shift = P.auto_table(vol)
    assert t.shift == shift == 0 and t.skipped == skipped == 0
    assert_tables_equal((t.hist, t.sum_s, t.skipped), (hist, sum_s, skipped))
    filled = t.counts > 0
    np.testing.assert_array_equal(t.means[filled], sum_s[filled] / (8.0 * hist.sum(axis=1)[filled]))
    assert np.isnan(t.means[~filled]).all()
    with DeviceImage(vol) as img:
        assert N.estimate_sigma(img) == P.estimate_sigma(vol)
    buf = ctx.to_device(vol)
    try:
        assert N.estimate_sigma(buf, shape=vol.shape, dtype=np.uint16) == P.estimate_sigma(vol)
        with pytest.raises(ValueError, match="shape"):
            N.estimate_sigma(buf)
    finally:
        buf.free()
    with pytest.raises(ValueError, match="3-D"):
        N.noise_table(vol[0])
    with pytest.raises(ValueError, match=">= 2"):
        N.noise_table(vol[:, :1])
    with pytest.raises(ValueError, match="shift"):
        N.noise_table(vol, shift=7)
    assert N.noise_table(vol.astype(np.float64)).hist.sum() == t.hist.sum()      # widened dtypes go as float32


def test_host_tensor_is_uploaded_not_dereferenced(ctx):
    """A torch tensor in host memory has a data_ptr, which is no device address: it goes the way of a numpy array."""
    torch = pytest.importorskip("torch")
    vol = volume((40, 36, 44), np.float32, seed=8)
    t = N.noise_table(torch.from_numpy(vol), shift=1)
    assert_tables_equal((t.hist, t.sum_s, t.skipped), P.table(vol, 1))
    assert N.estimate_sigma(torch.from_numpy(vol)) == P.estimate_sigma(vol)


def to_u16(x):
    return np.rint(np.clip(x, 0, 65535)).astype(np.uint16)


def ramp_volume(gain, read_noise, offset, seed=7, shape=(96, 96, 96)):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    u = (zz + yy + xx) / float(sum(shape) - 3)
    clean = 20.0 + 4000.0 * u * u
    return to_u16(gain * rng.poisson(clean / gain) + rng.normal(offset, read_noise, shape))


def test_estimators_equal_pyref_floats(ctx):
    rng = np.random.default_rng(1)
    flat = to_u16(1000.0 + rng.normal(0, 24.0, (64, 64, 64)))
    loud = to_u16(30000.0 + rng.normal(0, 3000.0, (32, 32, 32)))           # needs shift 1
    ramp = ramp_volume(2.0, 8.0, 100.0)
    f32 = volume((40, 36, 44), np.float32, seed=6)
    for vol in (flat, loud, ramp, f32):
        got = N.estimate_sigma(vol)
        assert got == P.estimate_sigma(vol) and math.isfinite(got)
        for a, b in zip(N.noise_curve(vol), P.noise_curve(vol)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(N.noise_curve(vol, min_cells=64), P.noise_curve(vol, min_cells=64)):
            np.testing.assert_array_equal(a, b)
    assert N.noise_table(loud).shift == 1
    small = to_u16(30000.0 + np.random.default_rng(5).normal(0, 3000.0, (8, 8, 16)))
    assert N.noise_table(small).shift == 1                 # no level has min_cells cells: the pooled row escalates
    assert N.estimate_sigma(small) == P.estimate_sigma(small) and math.isfinite(N.estimate_sigma(small))
    assert abs(N.estimate_sigma(flat) / math.sqrt(24.0 ** 2 + 1.0 / 12.0) - 1.0) <= 0.02
    assert N.estimate_poisson_gaussian(ramp, offset=100.0) == P.estimate_poisson_gaussian(ramp, 100.0)
    auto = N.estimate_poisson_gaussian(ramp)                                # offset from estimate_offset
    assert auto == P.estimate_poisson_gaussian(ramp, T.estimate_offset(ramp))
    with pytest.raises(ValueError, match="fewer than three"):
        N.estimate_poisson_gaussian(flat, offset=0.0)
    with pytest.raises(ValueError, match="slope"):
        N.fit_poisson_gaussian([10.0, 20.0, 30.0, 40.0], [4.0, 3.0, 2.0, 1.0], [1000] * 4, 0.0)
    board = np.zeros((8, 8, 8), dtype=np.uint16)
    zz, yy, xx = np.meshgrid(*[np.arange(8)] * 3, indexing="ij")
    board[(zz + yy + xx) % 2 == 0] = 65535
    assert math.isnan(N.estimate_sigma(board)) and N.noise_table(board).shift == 6
    with pytest.raises(ValueError, match="auto"):
        N.resolve_sigma("auto", board)
    with pytest.raises(ValueError, match="auto"):
        N.resolve_sigma("automatic", flat)


def test_anscombe_cfg_builds(ctx):
    ramp = ramp_volume(2.0, 8.0, 100.0)
    cfg = N.anscombe_cfg(ramp, offset=100.0)
    want = P.estimate_poisson_gaussian(ramp, 100.0)
    assert cfg == {"kind": "anscombe", "params": want}
    tf = T.build_transform(cfg)
    assert isinstance(tf, T.AnscombeTransform)
    assert (tf.gain, tf.read_noise, tf.offset) == (want["gain"], want["read_noise"], 100.0)
    assert abs(tf.gain / 2.0 - 1.0) <= 0.05 and abs(tf.read_noise / 8.0 - 1.0) <= 0.15


def test_bm4d_auto_sigma(ctx):
    z = synth_volume((32, 32, 32), seed=4, pedestal=300.0)[0]
    sigma = N.estimate_sigma(z)
    assert sigma == P.estimate_sigma(z) and 20.0 < sigma < 28.0
    np.testing.assert_array_equal(B.bm4d(z, "auto"), B.bm4d(z, sigma))
    batch = np.stack([synth_volume((16, 16, 16), seed=s, pedestal=300.0)[0] for s in range(3)])
    s4 = N.estimate_sigma(batch)
    np.testing.assert_array_equal(B.bm4d(batch, "auto"), B.bm4d(batch, s4))
    np.testing.assert_array_equal(B.denoise_patches(batch, "auto"), B.denoise_patches(batch, s4))
    with pytest.raises(ValueError, match="auto"):
        B.bm4d(z, "guess")


def test_denoise_volume_auto_sigma(ctx):
    v = synth_volume((32, 40, 48), seed=5, pedestal=300, as_u16=True)[0]
    sigma = N.estimate_sigma(v)
    assert sigma == P.estimate_sigma(v)
    np.testing.assert_array_equal(B.denoise_volume(v, "auto"), B.denoise_volume(v, sigma))
    np.testing.assert_array_equal(B.denoise_chunked(v, "auto", chunk=32), B.denoise_chunked(v, sigma, chunk=32))


def test_invalid_arguments(ctx):
    vol = volume((8, 8, 8), np.uint16)
    buf = ctx.to_device(vol)
    hist = np.zeros((P.LEVELS, P.BINS), np.uint64)
    sums = np.zeros(P.LEVELS, np.uint64)
    skipped = np.zeros(1, np.uint64)
    out = [a.ctypes.data_as(ctypes.c_void_p) for a in (hist, sums, skipped)]
    fn = nat.lib().exabm4d_noise_table_dev

    def refused(text, dtype=0, shape=(8, 8, 8), shift=0, ptr=buf.ptr, outs=out):
        assert fn(ctx.handle, ptr, dtype, *shape, shift, *outs) == -1          # EXABM4D_ERR_INVALID
        assert text in nat.lib().exabm4d_last_error(ctx.handle).decode()

    try:
        for dtype in (2, 3, -1):
            refused("uint16 or float32", dtype=dtype)
        for shift in (-1, 7):
            refused("shift must be 0..6", shift=shift)
            with pytest.raises(ValueError, match="shift must be 0..6"):
                ctx.noise_table(buf, np.uint16, (8, 8, 8), shift)
        for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (8, -2, 8)):
            refused("every extent must be >= 2", shape=shape)
            with pytest.raises(ValueError, match="extent"):
                ctx.noise_table(buf, np.uint16, shape, 0)
        refused("too large", shape=(1 << 20, 1 << 20, 2))
        refused("NULL", ptr=None)
        refused("NULL", outs=[out[0], None, out[2]])
        with pytest.raises(ValueError, match="uint16 or float32"):
            ctx.noise_table(buf, np.float64, (8, 8, 8), 0)
        assert hist.sum() == 0                                                  # nothing was written
        assert_tables_equal(ctx.noise_table(buf, np.uint16, (8, 8, 8), 0), P.table(vol, 0))    # and the context works
    finally:
        buf.free()
