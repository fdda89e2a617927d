"""Patch-cache mask builders and coherence gate on the MI355X (csrc/mask_kernels.hip) against the
reference's fixture (tests/golden/masks.npz) and against scipy.ndimage directly."""
import os

import numpy as np
import pytest

import mask_inputs as mi
from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression.machine_learning import metrics

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _unpack(golden, key, shape):
    return np.unpackbits(golden[key], count=int(np.prod(shape))).reshape(shape).astype(bool)


def test_foreground_masks_equal_the_fixture(golden):
    for name, (raw, k, dilate) in mi.foreground_cases().items():
        got = metrics.make_foreground_mask(raw, k=k, dilate=dilate)
        assert got.dtype == bool and got.shape == raw.shape
        assert np.array_equal(got, _unpack(golden, f"fg/{name}", raw.shape)), name


def test_foreground_thresholds_are_numpys_fp32_arithmetic():
    ctx = nat.context()
    for name, (raw, k, _) in mi.foreground_cases().items():
        r = np.asarray(raw, dtype=np.float32)
        med = np.median(r)
        mad = np.median(np.abs(r - med)) + 1e-6
        want = med + k * (1.4826 * mad)
        src = np.ascontiguousarray(raw)
        with ctx.to_device(src) as d, ctx.alloc(src.size) as m:
            thr = ctx.foreground_masks(d, src.dtype, 1, src.shape, k, 0, m)
        assert thr[0] == np.float32(want), name


def test_segmentation_and_skeleton_masks_equal_the_fixture(golden):
    for name, (labels, dilate) in mi.segmentation_cases().items():
        got = metrics.make_segmentation_mask(labels, dilate=dilate)
        assert np.array_equal(got, _unpack(golden, f"seg/{name}", labels.shape)), name
    for name, (pts, start, shape, dilate) in mi.skeleton_cases().items():
        got = metrics.make_skeleton_mask(pts, start, shape, dilate=dilate)
        assert np.array_equal(got, _unpack(golden, f"skel/{name}", shape)), name


def test_binary_dilation_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    shape = (9, 12, 7)
    seeds = np.zeros(shape, dtype=bool)
    seeds[0, 0, 0] = seeds[8, 11, 6] = seeds[0, 5, 3] = seeds[4, 11, 0] = seeds[8, 0, 6] = True   # corners, faces
    seeds |= rng.random(shape) < 0.01
    for k in range(6):
        want = ndimage.binary_dilation(seeds, iterations=k) if k else seeds
        got = metrics._dilate(seeds[None], k)[0]
        assert np.array_equal(got, want), k


def _gauss_dev(src, sigma):
    ctx = nat.context()
    src = np.ascontiguousarray(src)
    with ctx.to_device(src) as d, ctx.alloc(src.size * 8) as out:
        ctx.gaussian_filter3d(d, src.dtype, src.shape[0], src.shape[1:], metrics.gaussian_weights(sigma), out)
        return out.download(src.shape, np.float64)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 1.5, 2.0])
def test_gaussian_filter_equals_scipy_bit_for_bit(sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(sigma * 10))
    for shape in ((13, 17, 11), (5, 19, 3)):          # axes shorter than the radius (8 at sigma 2)
        batch = (rng.normal(100.0, 30.0, (3,) + shape)).astype(np.float32)
        got = _gauss_dev(batch, sigma)
        for b in range(3):
            want = ndimage.gaussian_filter(batch[b].astype(np.float64), sigma)
            assert np.array_equal(got[b], want), (shape, b)
        got64 = _gauss_dev(batch.astype(np.float64) * 1.1, sigma)
        assert np.array_equal(got64[1], ndimage.gaussian_filter(batch[1].astype(np.float64) * 1.1, sigma))


def test_scores_match_the_fixture(golden):
    for name, (raw, mask) in mi.score_cases().items():
        for lag in mi.LAGS:
            got = metrics.local_autocorr(raw, mask, lag=lag)
            assert abs(got - float(golden[f"ac/{name}/lag{lag}"])) <= 1e-10, (name, lag)
        got = metrics.highfreq_energy_fraction(raw, mask)
        assert abs(got - float(golden[f"hf/{name}"])) <= 1e-10, name


def test_highfreq_with_a_precomputed_smooth(golden):
    ndimage = pytest.importorskip("scipy.ndimage")
    raw, mask = mi.score_cases()["salt_pepper"]
    smooth = ndimage.gaussian_filter(raw.astype(np.float64), 1.0)
    got = metrics.highfreq_energy_fraction(raw, mask, smooth=smooth)
    assert abs(got - float(golden["hf/salt_pepper"])) <= 1e-10


def test_gate_decisions_equal_the_fixture(golden):
    for name, (labels, raw, min_vox) in mi.gate_cases().items():
        got = metrics.patch_has_incoherent_segment(labels, raw, min_segment_voxels=min_vox)
        assert isinstance(got, bool)
        assert got == bool(golden[f"gate/{name}"]), name


def test_label_set_overflow_falls_back_to_the_host():
    labels = mi.gate_cases()["overflow_20000"][0]
    ctx = nat.context()
    lab = np.ascontiguousarray(labels[None])
    with ctx.to_device(lab) as d:
        lists = metrics._label_lists(ctx, d, lab, 1, lab.shape[1:])
        _, _, held, status = ctx.label_set(d, lab.dtype, 1, lab.shape[1:])
    assert status[0] == 1 and held[0] <= nat.LABEL_SET_MAX
    u, c = np.unique(labels[labels > 0], return_counts=True)
    assert np.array_equal(lists[0][0], u) and np.array_equal(lists[0][1], c)


def test_label_set_equals_np_unique():
    for name, (labels, _, _) in mi.gate_cases().items():
        lab = metrics._labels_dev(labels[None])
        ctx = nat.context()
        with ctx.to_device(lab) as d:
            keys, counts = metrics._label_lists(ctx, d, lab, 1, lab.shape[1:])[0]
        u, c = np.unique(labels[labels > 0], return_counts=True)
        assert np.array_equal(keys, u.astype(np.uint64)) and np.array_equal(counts, c), name


def test_batched_equals_per_patch_and_is_deterministic(golden):
    names, labels, raw = mi.gate_batch()
    got = metrics.incoherent_segments(labels, raw)
    assert got.dtype == bool and got.shape == (len(names),)
    assert list(got) == [bool(golden[f"gate/{n}"]) for n in names]
    s1 = metrics.segment_scores(labels, raw)
    s2 = metrics.segment_scores(labels[::-1].copy(), raw[::-1].copy())[::-1]
    s3 = metrics.segment_scores(labels[2:3], raw[2:3])
    assert s1 == s2 and s1[2] == s3[0]                # same bits in any batch position
    for b in range(len(names)):
        assert metrics.segment_scores(labels[b:b + 1], raw[b:b + 1])[0] == s1[b]
    odd = mi.foreground_cases()["odd_k6_d1"][0]
    batch = np.stack([odd, odd[::-1].copy(), odd * 2.0])
    fg = metrics.foreground_masks(batch, 6.0, 1)
    for b in range(3):
        assert np.array_equal(fg[b], metrics.make_foreground_mask(batch[b], 6.0, 1))
    assert np.array_equal(fg, metrics.foreground_masks(batch, 6.0, 1))


def test_patch_cache_writer_builds_the_foreground_masks(tmp_path):
    from aind_exaspim_image_compression.machine_learning.data_handling import PatchCacheWriter
    rng = np.random.default_rng(11)
    raw = (rng.normal(20.0, 4.0, (3, 16, 16, 16)) + 300.0 * (rng.random((3, 16, 16, 16)) < 0.01)).astype(np.float32)
    with PatchCacheWriter(tmp_path, 3, patch_shape=(16, 16, 16), sigma_bm4d=4.0) as w:
        w.write(raw[:2])
        w.write(raw[2])
    fg = np.load(tmp_path / "fg.npy")
    for b in range(3):
        assert np.array_equal(fg[b], metrics.make_foreground_mask(raw[b]).astype(np.uint8))
