"""tests/mask_pyref.py, the plain reference of the mask kernels, checked without a GPU: against scipy.ndimage
bit for bit, against the committed fixture (tests/golden/masks.npz), and its exact segment statistics against
mask_inputs.segment_stats_np within the derived bound."""
import os

import numpy as np
import pytest

import mask_inputs as mi
import mask_pyref as P
from aind_exaspim_image_compression.machine_learning import metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks.npz")
SIGMAS = [0.0, 0.5, 1.0, 2.0, 3.7, 16.0]
SHAPES = [(1, 1, 1), (1, 2, 3), (5, 19, 3), (13, 17, 11), (3, 3, 200)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _unpack(golden, key, shape):
    return np.unpackbits(golden[key], count=int(np.prod(shape))).reshape(shape).astype(bool)


def test_dilate_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for shape in [(1, 1, 1), (1, 1, 9), (2, 1, 5), (1, 7, 2), (2, 2, 2), (9, 12, 7)]:
        seeds = rng.random(shape) < 0.08
        seeds[0, 0, 0] = seeds[-1, -1, -1] = True
        assert np.array_equal(P.dilate(seeds, 0), seeds)
        for k in range(1, 9):
            assert np.array_equal(P.dilate(seeds, k), ndimage.binary_dilation(seeds, iterations=k)), (shape, k)
    bytes_ = (rng.random((4, 5, 6)) < 0.1) * rng.integers(2, 256, (4, 5, 6))        # non-0 bytes other than 1
    assert np.array_equal(P.dilate(bytes_.astype(np.uint8), 2), ndimage.binary_dilation(bytes_ != 0, iterations=2))


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_equals_scipy_bit_for_bit(sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(sigma * 10))
    w = metrics.gaussian_weights(sigma)
    assert len(w) - 1 == (int(4.0 * sigma + 0.5) if sigma else 0)
    for shape in SHAPES:
        x = rng.normal(100.0, 30.0, shape)
        for src in (x.astype(np.float32), x):
            want = ndimage.gaussian_filter(src.astype(np.float64), sigma)
            np.testing.assert_array_equal(P.gaussian(src, w), want, err_msg=str((sigma, shape, src.dtype)))


def test_reflect_is_scipys_reflect_at_any_distance():
    for n in (1, 2, 3, 7):
        row = np.arange(n)
        want = np.pad(row, 70, mode="symmetric")       # numpy's "symmetric" is scipy's "reflect"
        np.testing.assert_array_equal(P.reflect(np.arange(-70, n + 70), n), want)


def test_foreground_masks_equal_the_fixture(golden):
    for name, (raw, k, dilate) in mi.foreground_cases().items():
        assert np.array_equal(P.fg_mask(raw, k, dilate), _unpack(golden, f"fg/{name}", raw.shape)), name


def test_threshold_is_nan_where_numpys_is():
    r = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    assert P.fg_threshold(r, 6.0) == np.float32(13.0 + 6.0 * np.float32(1.4826 * np.float32(7.0 + 1e-6)))
    for bad in (np.nan, -np.nan):
        q = r.copy()
        q[1, 1, 1] = bad
        assert np.isnan(P.fg_threshold(q, 6.0)) and not P.fg_mask(q, 6.0, 2).any()
    q = r.copy()
    q[:2] = np.inf                                         # the median is +inf: inf - inf is NaN
    assert np.isnan(P.fg_threshold(q, 6.0)) and not P.fg_mask(q, 6.0, 0).any()
    q = r.copy()
    q[0, 0, :2] = [np.inf, -np.inf]                        # a few infinities among finite data: nothing special
    assert np.isfinite(P.fg_threshold(q, 6.0)) and P.fg_mask(q, 0.0, 0).sum() == 13


def test_segmentation_and_skeleton_masks_equal_the_fixture(golden):
    for name, (labels, dilate) in mi.segmentation_cases().items():
        assert np.array_equal(P.dilate(labels > 0, dilate), _unpack(golden, f"seg/{name}", labels.shape)), name
    for name, (pts, start, shape, dilate) in mi.skeleton_cases().items():
        inside = np.all((pts >= start) & (pts < start + np.asarray(shape)), axis=1)
        local = (pts[inside] - start).astype(int)
        mask = np.zeros(shape, dtype=bool)
        mask[local[:, 0], local[:, 1], local[:, 2]] = True
        assert np.array_equal(P.dilate(mask, dilate), _unpack(golden, f"skel/{name}", shape)), name


def test_label_counts_and_segment_mask():
    lab = np.array([[[-3, 0, 5, 5, 2, -3, 2, 5]]], dtype=np.int32)
    u, c = P.label_counts(lab)
    assert list(u) == [2, 5] and list(c) == [2, 3]
    assert P.segment_mask(lab, 5).sum() == 3 and not P.segment_mask(lab, 0).any()
    assert not P.segment_mask(lab, 2 ** 40).any() and not P.segment_mask(lab.astype(np.uint8), 256 + 5).any()
    big = np.array([[[2 ** 63, 2 ** 64 - 1, 0]]], dtype=np.uint64)
    assert P.segment_mask(big, 2 ** 64 - 1).tolist() == [[[False, True, False]]]


def test_exact_statistics_of_a_hand_case():
    lab = np.zeros((1, 2, 4), dtype=np.uint8)
    raw = np.array([[[1.0, 2.0, 4.0, 8.0], [3.0, 5.0, 7.0, 9.0]]])
    lab[0, 0, :] = 1
    lab[0, 1, 0] = 1                        # the voxel after the row end: no pair along x may reach it
    st = P.segment_stats_exact(lab, 1, raw, 1, raw - 0.5)
    assert st[0] == 5 and st[1] == 3.6 and st[2] == 0.5 and st[4] == 0.0
    assert st[3] == pytest.approx(29.2, abs=1e-13)
    assert list(st[5:11]) == [0.0] * 6                                   # one plane
    assert list(st[11:17]) == [1.0, 1.0, 3.0, 0.0, 0.0, 0.0]              # (0,0,0)-(0,1,0)
    n, mx, my, sxx, syy, sxy = st[17:23]
    assert (n, mx, my) == (3.0, 7.0 / 3.0, 14.0 / 3.0)
    assert sxx == pytest.approx(14.0 / 3.0, abs=1e-15) and syy == pytest.approx(56.0 / 3.0, abs=1e-14)
    assert sxy == pytest.approx(28.0 / 3.0, abs=1e-14)
    assert not P.segment_stats_exact(lab, 1, raw, 4)[5:].any() and not P.segment_stats_exact(lab, 0, raw, 1).any()


def test_exact_statistics_against_numpy_within_the_bound():
    """segment_stats_np sums pairwise in fp64: one more summation order the bound must hold for."""
    worst = {}
    for name, (raw, mask) in mi.score_cases().items():
        r64 = np.asarray(raw, dtype=np.float64)
        lab = mask.astype(np.uint8)
        smooth = P.gaussian(r64, metrics.gaussian_weights(1.0))
        for lag, sm in [(lag, None) for lag in mi.LAGS] + [(1, smooth)]:
            want = P.segment_stats_exact(lab, 1, r64, lag, sm)
            bound = P.segment_stats_bound(lab, 1, r64, lag, sm)
            worst[name] = max(worst.get(name, 0.0),
                              P.check_stats(mi.segment_stats_np(r64, mask, lag, sm), want, bound, f"{name} lag {lag}"))
    print("error / bound of the numpy two-pass sums:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_the_bound_catches_the_one_pass_formula():
    raw, mask = mi.score_cases()["offset_60000"]
    r64 = np.asarray(raw, dtype=np.float64)
    v = r64[mask]
    one_pass = float(np.sum(v * v) - v.size * v.mean() ** 2)
    lab = mask.astype(np.uint8)
    want, bound = P.segment_stats_exact(lab, 1, r64, 1), P.segment_stats_bound(lab, 1, r64, 1)
    assert abs(one_pass - want[3]) > 1000 * bound[3]


def test_finishing_rules_on_the_exact_statistics_reproduce_the_fixture(golden):
    for name, (raw, mask) in mi.score_cases().items():
        r64 = np.asarray(raw, dtype=np.float64)
        lab = mask.astype(np.uint8)
        for lag in mi.LAGS:
            st = P.segment_stats_exact(lab, 1, r64, lag)
            assert abs(metrics.autocorr_from_stats(st) - float(golden[f"ac/{name}/lag{lag}"])) <= 1e-12, (name, lag)
        st = P.segment_stats_exact(lab, 1, r64, 1, P.gaussian(r64, metrics.gaussian_weights(1.0)))
        assert abs(metrics.highfreq_from_stats(st) - float(golden[f"hf/{name}"])) <= 1e-12, name
