"""Host side of the patch-cache mask builders and coherence gate (CPU): the fixture and its seeded
inputs, the Gaussian weights, the finishing rules applied to segment sums, argument checks, and
the loud failure without a GPU."""
import os

import numpy as np
import pytest

import mask_inputs as mi
from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression.machine_learning import metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_present_and_inputs_regenerate(golden):
    assert str(golden["inputs_sha256"]) == mi.inputs_digest()
    keys = set(golden.files)
    for prefix, cases in (("fg", mi.foreground_cases()), ("seg", mi.segmentation_cases()),
                          ("skel", mi.skeleton_cases()), ("gate", mi.gate_cases())):
        for name in cases:
            assert f"{prefix}/{name}" in keys
    for name in mi.score_cases():
        assert f"hf/{name}" in keys
        for lag in mi.LAGS:
            assert f"ac/{name}/lag{lag}" in keys


def test_fixture_covers_the_decisions(golden):
    gate = {n: bool(golden[f"gate/{n}"]) for n in mi.gate_cases()}
    assert gate["salt_pepper_flagged"] and gate["overflow_20000"] and gate["u64_big_ids"]
    assert not (gate["blob_kept"] or gate["empty"] or gate["speck_27_ignored"]
                or gate["i32_negative_ids"] or gate["u64_big_ids_blob_only"])
    labels = mi.gate_cases()["overflow_20000"][0]
    assert len(np.unique(labels[labels > 0])) > nat.LABEL_SET_MAX


@pytest.mark.parametrize("sigma", [0.5, 1.0, 1.5, 2.0, 3.7, 1])
def test_gaussian_weights_equal_scipy(sigma):
    ndimage_filters = pytest.importorskip("scipy.ndimage._filters")
    radius = int(4.0 * float(sigma) + 0.5)
    want = ndimage_filters._gaussian_kernel1d(sigma, 0, radius)[::-1]
    got = metrics.gaussian_weights(sigma)
    assert got.dtype == np.float64 and len(got) == radius + 1
    assert np.array_equal(got, want[radius:])
    assert np.array_equal(want[:radius + 1][::-1], want[radius:])    # symmetric bit for bit
    assert np.array_equal(metrics.gaussian_weights(0.0), [1.0])


def test_finishing_rules_reproduce_the_fixture(golden):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, (raw, mask) in mi.score_cases().items():
        r64 = np.asarray(raw, dtype=np.float64)
        smooth = ndimage.gaussian_filter(r64, 1.0)
        for lag in mi.LAGS:
            st = mi.segment_stats_np(r64, mask, lag)
            assert abs(metrics.autocorr_from_stats(st) - float(golden[f"ac/{name}/lag{lag}"])) <= 1e-12, (name, lag)
        st = mi.segment_stats_np(r64, mask, 1, smooth)
        assert abs(metrics.highfreq_from_stats(st) - float(golden[f"hf/{name}"])) <= 1e-12, name


def test_finishing_rules_reproduce_the_gate_decisions(golden):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, (labels, raw, min_vox) in mi.gate_cases().items():
        r64 = np.asarray(raw, dtype=np.float64)
        smooth = ndimage.gaussian_filter(r64, 1.0)
        flagged = False
        for lid in np.unique(labels[labels > 0]):
            seg = labels == lid
            if seg.sum() < min_vox:
                continue
            ac = metrics.autocorr_from_stats(mi.segment_stats_np(r64, seg, 2))
            hf = metrics.highfreq_from_stats(mi.segment_stats_np(r64, seg, 2, smooth))
            flagged |= (not ac >= 0.4) and hf > 0.35
        assert flagged == bool(golden[f"gate/{name}"]), name


def _row(n=100.0, ss_raw=50.0, ss_hf=10.0, axes=((100.0, 1.0, 2.0, 4.0, 9.0, 3.0),) * 3):
    return np.array([n, 0.0, 0.0, ss_raw, ss_hf] + [v for ax in axes for v in ax])


def test_finishing_rule_branches():
    # every axis measurable: mean of Pearson correlations, clipped to [-1, 1]
    assert metrics.autocorr_from_stats(_row()) == pytest.approx(0.5, abs=1e-15)
    over = _row(axes=((10.0, 0, 0, 1.0, 1.0, 1.0 + 1e-9),) * 3)
    assert metrics.autocorr_from_stats(over) == 1.0
    # fewer than 2 pairs, or a std below 1e-6: the axis is skipped
    skipped = _row(axes=((1.0, 0, 0, 4.0, 9.0, 6.0), (100.0, 0, 0, 1e-11, 9.0, 0.0),
                         (100.0, 0, 0, 4.0, 9.0, -3.0)))
    assert metrics.autocorr_from_stats(skipped) == pytest.approx(-0.5, abs=1e-15)
    # no axis counts: 1.0
    none = _row(axes=((0.0, 0, 0, 0, 0, 0), (1.0, 0, 0, 4.0, 9.0, 6.0), (50.0, 0, 0, 0.0, 9.0, 0.0)))
    assert metrics.autocorr_from_stats(none) == 1.0
    # high-frequency fraction: ratio of variances, 0.0 below 1e-12, NaN for an empty mask
    assert metrics.highfreq_from_stats(_row()) == pytest.approx(0.2, abs=1e-15)
    assert metrics.highfreq_from_stats(_row(ss_raw=1e-11)) == 0.0
    assert np.isnan(metrics.highfreq_from_stats(_row(n=0.0)))


def test_argument_checks_come_before_the_device():
    with pytest.raises(ValueError):
        metrics.make_foreground_mask(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        metrics.foreground_masks(np.zeros((4, 4, 4), np.float32))
    with pytest.raises(ValueError):
        metrics.incoherent_segments(np.zeros((2, 4, 4, 4), np.int32), np.zeros((2, 4, 4, 5)))
    with pytest.raises(ValueError):
        metrics.patch_has_incoherent_segment(np.zeros((4, 4, 4, 1), np.int32), np.zeros((4, 4, 4, 1)))
    with pytest.raises(ValueError):
        metrics.incoherent_segments(np.zeros((1, 4, 4, 4), np.float32), np.zeros((1, 4, 4, 4)))
    with pytest.raises(ValueError):
        metrics.local_autocorr(np.zeros((4, 4, 4)), np.zeros((4, 4, 5), bool))
    with pytest.raises(ValueError):
        metrics.make_segmentation_mask(np.zeros((0, 4, 4), np.int32))
    assert metrics.foreground_masks(np.zeros((0, 4, 4, 4), np.float32)).shape == (0, 4, 4, 4)
    assert metrics.incoherent_segments(np.zeros((0, 4, 4, 4), np.int32),
                                       np.zeros((0, 4, 4, 4))).shape == (0,)


def test_mask_builders_fail_loudly_without_a_gpu():
    if nat.device_count() > 0:
        pytest.skip("a GPU is visible")
    raw = np.ones((6, 6, 6), np.float32)
    labels = np.ones((6, 6, 6), np.int32)
    calls = [
        lambda: metrics.make_foreground_mask(raw),
        lambda: metrics.foreground_masks(raw[None]),
        lambda: metrics.local_autocorr(raw, labels > 0),
        lambda: metrics.highfreq_energy_fraction(raw, labels > 0),
        lambda: metrics.make_segmentation_mask(labels, dilate=1),
        lambda: metrics.make_skeleton_mask(np.zeros((1, 3)), (0, 0, 0), (6, 6, 6)),
        lambda: metrics.patch_has_incoherent_segment(labels, raw),
        lambda: metrics.incoherent_segments(labels[None], raw[None]),
    ]
    for call in calls:
        with pytest.raises(nat.NativeError):
            call()
