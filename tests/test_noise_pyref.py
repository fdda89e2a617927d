"""The noise estimator itself, pinned on its numpy restatement (tests/noise_pyref.py; CPU only): how close the
pooled sigma and the Poisson-Gaussian fit come on fixed inputs, and the exact cases of the table's definition
(DESIGN.md 5.9).  Every input and seed is fixed; the bounds are conditions on these inputs."""
import math

import numpy as np
import pytest

import noise_pyref as P
from util import synth_volume


def to_u16(x):
    return np.rint(np.clip(x, 0, 65535)).astype(np.uint16)


def ramp(shape=(96, 96, 96)):
    """A smooth quadratic ramp 20 .. 4020 counts along the volume's diagonal."""
    zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    u = (zz + yy + xx) / float(sum(shape) - 3)
    return 20.0 + 4000.0 * u * u


def poisson_gaussian_volume(gain, read_noise, offset, seed):
    rng = np.random.default_rng(seed)
    clean = ramp()
    return to_u16(gain * rng.poisson(clean / gain) + rng.normal(offset, read_noise, clean.shape))


@pytest.mark.parametrize("sigma", [2, 5, 24, 60, 200])
def test_pooled_sigma_on_a_flat_field(sigma):
    rng = np.random.default_rng(100 + sigma)
    vol = to_u16(1000.0 + rng.normal(0, sigma, (64, 64, 64)))
    want = math.sqrt(sigma ** 2 + 1.0 / 12.0)      # the rounding to whole counts is part of the stored noise
    got = P.estimate_sigma(vol)
    print(f"flat field sigma {sigma}: estimate {got:.4f}, want {want:.4f}, error {100 * (got / want - 1):+.2f} %")
    assert abs(got / want - 1.0) <= 0.02


@pytest.mark.parametrize("sigma", [24, 60])
def test_pooled_sigma_on_the_synthetic_volume(sigma):
    """Pedestal 300, not the default 37: at 37 the uint16 clip at 0 removes 6 % of the voxels at sigma 24 and the
    estimate correctly reads 23.0."""
    vol, _ = synth_volume((96, 96, 96), seed=3, sigma=float(sigma), pedestal=300, as_u16=True)
    want = math.sqrt(sigma ** 2 + 1.0 / 12.0)
    got = P.estimate_sigma(vol)
    print(f"synthetic volume sigma {sigma}: estimate {got:.4f}, error {100 * (got / want - 1):+.2f} %")
    assert abs(got / want - 1.0) <= 0.02


@pytest.mark.parametrize("gain,read_noise,offset", [(2, 8, 100), (0.5, 3, 37), (4, 20, 200)])
def test_poisson_gaussian_fit_on_a_smooth_ramp(gain, read_noise, offset):
    vol = poisson_gaussian_volume(gain, read_noise, offset, seed=7)
    got = P.estimate_poisson_gaussian(vol, offset)
    print(f"gain {gain} read noise {read_noise} offset {offset}: gain {got['gain']:.4f} "
          f"({100 * (got['gain'] / gain - 1):+.2f} %), read noise {got['read_noise']:.4f} "
          f"({100 * (got['read_noise'] / read_noise - 1):+.2f} %)")
    assert abs(got["gain"] / gain - 1.0) <= 0.05
    assert abs(got["read_noise"] / read_noise - 1.0) <= 0.15
    assert got["offset"] == offset


def test_level_at_every_octave_edge():
    mean = np.array([0, 15, 16, 47, 48, 65535], dtype=np.int64)
    want = [0, 3, 4, 7, 8, 48]
    for low in (0, 7):                                   # s >> 3 drops the low three bits
        assert list(P.level_of(8 * mean + low)) == want
    for m, lv in zip(mean, want):                        # and through the table: a constant cell has d = 0
        hist, sum_s, skipped = P.table(np.full((2, 2, 2), m, dtype=np.uint16))
        assert hist[lv, 0] == 1 and hist.sum() == 1 and sum_s[lv] == 8 * m and sum_s.sum() == 8 * m and skipped == 0
    assert P.level_of(np.arange(0, P.S_MAX + 1)).max() == P.LEVELS - 1


def test_one_cell_by_hand():
    vol = np.array([[[1, 2], [3, 4]], [[5, 6], [7, 70]]], dtype=np.uint16)
    s, m, valid = P.cell_values(vol)
    assert s[0] == 98 and m[0] == abs(1 - 2 - 3 + 4 - 5 + 6 + 7 - 70) and valid.all()
    hist, sum_s, _ = P.table(vol, 2)
    assert hist[P.level_of(98), 62 >> 2] == 1 and hist.sum() == 1
    f = P.table(vol.astype(np.float32), 2)
    assert np.array_equal(f[0], hist) and np.array_equal(f[1], sum_s)


def test_odd_extents_are_ignored():
    vol, _ = synth_volume((33, 31, 36), seed=1, as_u16=True)
    odd = vol[:, :, :35]
    for a, b in zip(P.table(odd), P.table(np.ascontiguousarray(vol[:32, :30, :34]))):
        assert np.array_equal(a, b)
    assert P.table(odd)[0].sum() == 16 * 15 * 17


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_shift_folds_the_table(dtype):
    vol, _ = synth_volume((32, 32, 32), seed=2, sigma=800.0, pedestal=2000, as_u16=True)
    vol = vol.astype(dtype)
    s, m, valid = P.cell_values(vol)
    assert m.max() >= P.BINS                             # the clamp to the last bin takes part
    lv = P.level_of(s)
    base = P.table(vol, 0)
    for k in range(7):
        hist, sum_s, skipped = P.table(vol, k)
        want = np.zeros_like(hist)
        np.add.at(want, (lv, np.minimum(m >> k, P.BINS - 1)), 1)
        assert np.array_equal(hist, want)
        assert np.array_equal(sum_s, base[1]) and skipped == 0
        if m.max() >> k < P.BINS:                        # nothing clamped: the shift-0 ... table re-binned
            fine = np.zeros((P.LEVELS, P.BINS << k), dtype=np.uint64)
            np.add.at(fine, (lv, m), 1)
            assert np.array_equal(hist, fine.reshape(P.LEVELS, P.BINS, 1 << k).sum(axis=2))
    quiet, _ = synth_volume((32, 32, 32), seed=2, as_u16=True)        # sigma 24: no cell reaches the last bin
    quiet = quiet.astype(dtype)
    h0 = P.table(quiet, 0)[0]
    assert h0[:, -1].sum() == 0
    for k in range(1, 7):
        folded = h0.reshape(P.LEVELS, P.BINS >> k, 1 << k).sum(axis=2)
        hk = P.table(quiet, k)[0]
        assert np.array_equal(hk[:, :P.BINS >> k], folded) and hk[:, P.BINS >> k:].sum() == 0


def test_fp32_cells_that_are_not_finite_are_skipped():
    vol, _ = synth_volume((16, 16, 16), seed=4, pedestal=5.0)        # float32, negative counts among them
    assert (vol < 0).any()
    clean = P.table(vol)
    bad = vol.copy()
    bad[3, 4, 5] = np.nan
    bad[8, 9, 10] = np.inf
    bad[8, 9, 11] = np.inf                                           # the same cell: s = inf, d = nan
    bad[12, 0, 0] = -np.inf
    hist, sum_s, skipped = P.table(bad)
    assert skipped == 3 and hist.sum() == clean[0].sum() - 3
    keep = vol.copy()
    for z, y, x in ((2, 4, 4), (8, 8, 10), (12, 0, 0)):              # the same table without those three cells
        keep[z:z + 2, y:y + 2, x:x + 2] = np.nan
    assert np.array_equal(P.table(keep)[0], hist) and np.array_equal(P.table(keep)[1], sum_s)


def test_median_interpolation_and_the_saturated_row():
    row = np.zeros(P.BINS, dtype=np.uint64)
    row[0] = 10                                          # bin 0 of shift 0 covers [0, 0.5)
    assert P.sigma_of(row, 0) == 0.25 / P.MAD_TO_SIGMA
    row[:] = 0
    row[3], row[4] = 6, 2                                # n / 2 = 4 of the 6 in [2.5, 3.5)
    assert P.sigma_of(row, 0) == (2.5 + 4.0 / 6.0) / P.MAD_TO_SIGMA
    assert P.sigma_of(row, 2) == (11.5 + 4.0 / 6.0 * 4.0) / P.MAD_TO_SIGMA
    row[:] = 0
    assert math.isnan(P.sigma_of(row, 0))
    row[-1], row[7] = 5, 4
    assert math.isnan(P.sigma_of(row, 0))                # the median lies in the last bin
    row[7] = 5
    assert P.sigma_of(row, 0) == 7.5 / P.MAD_TO_SIGMA    # exactly half below it: the upper edge of bin 7
    board = np.zeros((8, 8, 8), dtype=np.uint16)
    zz, yy, xx = np.meshgrid(*[np.arange(8)] * 3, indexing="ij")
    board[(zz + yy + xx) % 2 == 0] = 65535              # |d| = 4 * 65535 in every cell, beyond every shift
    hist, _, _, shift = P.auto_table(board)
    assert shift == 6 and hist[:, -1].sum() == 64
    assert math.isnan(P.estimate_sigma(board))
    assert len(P.noise_curve(board, min_cells=1)[0]) == 0


def test_auto_shift_stops_at_the_first_unsaturated_table():
    """sigma 3000: the median of |d| is 0.6745 sqrt(8) 3000 = 5723, beyond the 4095 of shift 0 and well inside the
    8190 of shift 1.  The median of n = 4096 half-normal samples has a relative standard error of 1.17 / sqrt(n) =
    1.8 %; the bound is five of them."""
    rng = np.random.default_rng(5)
    vol = to_u16(30000.0 + rng.normal(0, 3000.0, (32, 32, 32)))
    assert math.isnan(P.sigma_of(P.table(vol, 0)[0].sum(axis=0), 0))
    hist, _, _, shift = P.auto_table(vol)
    assert shift == 1
    assert abs(P.sigma_of(hist.sum(axis=0), shift) / 3000.0 - 1.0) < 0.09


def test_auto_shift_follows_the_pooled_row_too():
    """128 cells, spread over several levels: no level reaches min_cells, so the levels alone would leave the table
    at shift 0, where the pooled median (5723) lies in the last bin and estimate_sigma would be NaN.  The pooled row
    is the one estimate_sigma reads, so it escalates like a level does."""
    rng = np.random.default_rng(5)
    vol = to_u16(30000.0 + rng.normal(0, 3000.0, (8, 8, 16)))
    hist = P.table(vol, 0)[0]
    assert hist.sum(axis=1).max() < 512 and math.isnan(P.sigma_of(hist.sum(axis=0), 0))
    assert P.auto_table(vol)[3] == 1
    assert 2000.0 < P.estimate_sigma(vol) < 4000.0       # 128 cells: a median with 10 % standard error, and finite


def test_fit_errors_say_which():
    rng = np.random.default_rng(6)
    flat = to_u16(1000.0 + rng.normal(0, 5.0, (32, 32, 32)))         # one or two levels only
    with pytest.raises(ValueError, match="fewer than three"):
        P.estimate_poisson_gaussian(flat, 0.0)
    with pytest.raises(ValueError, match="slope"):
        P.fit_poisson_gaussian([10.0, 20.0, 30.0, 40.0], [4.0, 3.0, 2.0, 1.0], [1000] * 4, 0.0)
    with pytest.raises(ValueError, match="fewer than three"):
        P.fit_poisson_gaussian([10.0, 20.0, 30.0], [0.0, 3.0, 4.0], [1000] * 3, 0.0)     # sigma 0 has no weight
    ok = P.fit_poisson_gaussian([10.0, 20.0, 30.0], [math.sqrt(14.0), math.sqrt(24.0), math.sqrt(34.0)], [1000] * 3, 2.0)
    assert abs(ok["gain"] - 1.0) < 1e-12 and abs(ok["read_noise"] - math.sqrt(6.0)) < 1e-12
