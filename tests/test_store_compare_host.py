"""The host side of ``evaluate.compare_stores``, without a GPU: the brick plan, what the host derives
from a signed difference table, and ``img_util.mip_to_uint8``, against numpy."""
import math

import numpy as np
import pytest

import compare_pyref as ref
from aind_exaspim_image_compression.utils import img_util, store_compare
from aind_exaspim_image_compression.utils.store_compare import (READER_SHARE, abs_error_percentile, error_stats,
                                                                halo_range, plan_compare, window_slabs)

# (shape, chunks, window, budget, with_mask): odd sizes, a volume of one chunk, an axis shorter than the window (whole,
# reflected more than once), window 1 (no halo), budgets from "one chunk" to "everything"
PLANS = [
    ((45, 38, 52), (16, 16, 32), 16, 1, False),
    ((45, 38, 52), (16, 16, 32), 16, 300_000, True),
    ((45, 38, 52), (16, 16, 32), 7, 150_000, False),
    ((45, 38, 52), (16, 16, 32), 16, 1 << 30, True),
    ((10, 40, 70), (4, 16, 32), 16, 120_000, False),
    ((5, 6, 7), (8, 8, 8), 16, 1, False),
    ((33, 17, 64), (8, 8, 8), 1, 40_000, False),
    ((100, 90, 80), (32, 32, 32), 32, 2_000_000, True),
]


@pytest.mark.parametrize("shape, chunks, window, budget, with_mask", PLANS)
def test_plan_compare(shape, chunks, window, budget, with_mask):
    bricks = plan_compare(shape, chunks, window, budget, with_mask)
    assert bricks == plan_compare(shape, chunks, window, budget, with_mask)            # deterministic
    # the bricks partition the volume, in raster order, and are boxes of whole chunks cut at the faces
    seen = np.zeros(shape, np.int32)
    for b in bricks:
        seen[ref.box_slices(b.origin, b.extent)] += 1
        for o, e, c, s in zip(b.origin, b.extent, chunks, shape):
            assert o % c == 0 and (e % c == 0 or o + e == s) and e >= 1
    assert np.all(seen == 1)
    assert [b.origin for b in bricks] == sorted(b.origin for b in bricks)
    stores = 3 if with_mask else 2
    single = tuple(min(c, s) for c, s in zip(chunks, shape))
    for b in bricks:
        for a in range(3):
            lo, n = b.win_origin[a], b.win_extent[a]
            assert 0 <= lo and lo + n <= shape[a]
            # the window holds every sample the brick's SSIM reads, after reflection ...
            need = ref.ssim_samples(b.origin[a], b.extent[a], shape[a], window)
            assert min(need) >= lo and max(need) < lo + n
            assert (lo, n) == (min(need), max(need) - min(need) + 1) or shape[a] < window
            # ... and an axis shorter than the window is there whole
            if shape[a] < window:
                assert (lo, n) == (0, shape[a])
        slabs, slab = window_slabs(b.win_extent[0], chunks[0])
        assert b.cost == stores * (2 * slabs * slab * b.win_extent[1] * b.win_extent[2] + budget // READER_SHARE)
        assert b.cost <= budget or all(e <= s for e, s in zip(b.extent, single))
        assert b.window_voxels == int(np.prod(b.win_extent))


def test_plan_compare_budget_decides_the_brick_count():
    shape, chunks = (45, 38, 52), (16, 16, 32)
    assert len(plan_compare(shape, chunks, 16, 1)) == 3 * 3 * 2
    assert len(plan_compare(shape, chunks, 16, 1 << 30)) == 1
    counts = [len(plan_compare(shape, chunks, 16, b)) for b in (1, 200_000, 250_000, 400_000, 1 << 30)]
    assert counts == sorted(counts, reverse=True) and 1 < counts[2] < 18
    for bad in [dict(window=0), dict(window=33), dict(budget_bytes=0), dict(shape=(4, 4)), dict(chunks_zyx=(0, 4, 4))]:
        kw = dict(shape=shape, chunks_zyx=chunks, window=16, budget_bytes=1000)
        kw.update(bad)
        with pytest.raises(ValueError):
            plan_compare(**kw)


def test_halo_range_is_the_hull_of_the_reflected_samples():
    for n in (1, 2, 5, 7, 16, 17, 40):
        for window in (1, 2, 7, 16, 32):
            for b0 in range(n):
                for bd in range(1, n - b0 + 1):
                    need = ref.ssim_samples(b0, bd, n, window)
                    lo, ext = halo_range(b0, bd, n, window)
                    if n < window:
                        assert (lo, ext) == (0, n)
                    else:
                        assert (lo, ext) == (min(need), max(need) - min(need) + 1), (n, window, b0, bd)


def _table_of(a, b):
    return ref.diff_table(a, b, (0, 0, 0), a.shape)


@pytest.mark.parametrize("kind", ["synth", "full_range", "equal", "one_voxel"])
def test_error_stats_and_percentiles_against_numpy(kind):
    shape = (9, 14, 23)
    if kind == "synth":
        a, b = ref.synth_pair(shape)
    elif kind == "full_range":
        a, b = ref.full_range_pair(shape, 5)
    elif kind == "equal":
        a, _ = ref.synth_pair(shape)
        b = a.copy()
    else:
        a, b = np.array([[[7]]], np.uint16), np.array([[[65535]]], np.uint16)
    hist = _table_of(a, b)
    d = b.astype(np.int64) - a.astype(np.int64)
    got = error_stats(hist, data_range=1234.5)
    n = d.size
    assert got["n"] == n and got["lmax"] == int(np.abs(d).max())
    # integer sums and one division: numpy's int64 sums are exact at this size, so the quotients are equal
    assert got["mae"] == int(np.abs(d).sum()) / n
    assert got["mse"] == int((d * d).sum()) / n
    assert got["bias"] == int(d.sum()) / n
    if kind == "equal":
        assert got["psnr"] == float("inf") and got["mae"] == 0.0 and got["lmax"] == 0
    else:
        assert got["psnr"] == 10.0 * math.log10(1234.5 ** 2 / got["mse"])
    assert "psnr" not in error_stats(hist)
    for q in (0, 0.1, 1, 25, 50, 75, 99, 99.9, 100, 33.3333):
        assert abs_error_percentile(hist, q) == ref.abs_percentile(a, b, q), q
    with pytest.raises(ValueError):
        abs_error_percentile(hist, 100.5)
    with pytest.raises(ValueError):
        error_stats(hist[:-1])


def test_error_stats_do_not_overflow():
    """10^12 voxels at the ends of the range: the sums pass 2^64, Python's integers hold them."""
    hist = np.zeros(ref.DIFF_BINS, np.uint64)
    hist[0], hist[-1], hist[65535] = 4 * 10 ** 11, 5 * 10 ** 11, 10 ** 11
    got = error_stats(hist)
    assert got["n"] == 10 ** 12 and got["lmax"] == 65535
    assert got["mae"] == (9 * 10 ** 11 * 65535) / 10 ** 12
    assert got["mse"] == (9 * 10 ** 11 * 65535 ** 2) / 10 ** 12
    assert got["bias"] == (10 ** 11 * 65535) / 10 ** 12
    assert abs_error_percentile(hist, 5) == 0.0 and abs_error_percentile(hist, 50) == 65535.0
    empty = error_stats(np.zeros(ref.DIFF_BINS, np.uint64))
    assert empty["n"] == 0 and math.isnan(empty["mae"]) and empty["lmax"] == 0
    assert math.isnan(abs_error_percentile(np.zeros(ref.DIFF_BINS, np.uint64), 50))


def test_mip_to_uint8():
    a, b = ref.synth_pair((12, 33, 41), seed=2)
    planes = [a.max(axis=0), b.max(axis=1), np.abs(a.astype(np.int32) - b).max(axis=2).astype(np.uint16)]
    planes.append(np.full((5, 9), 300, np.uint16))            # hi <= lo: a flat plane
    planes.append(np.zeros((4, 4), np.uint16))
    flat_but_one = np.full((40, 50), 17, np.uint16)           # both percentiles on the plateau, one voxel above it
    flat_but_one[3, 4] = 9000
    planes.append(flat_but_one)
    for p in planes:
        for pct in ((1.0, 99.9), (0.0, 100.0), (5.0, 50.0)):
            got = img_util.mip_to_uint8(p, *pct)
            assert got.dtype == np.uint8 and got.shape == p.shape
            np.testing.assert_array_equal(got, ref.mip_to_uint8(p, *pct))
    assert np.all(img_util.mip_to_uint8(planes[3]) == 0)
    assert img_util.mip_to_uint8(flat_but_one)[3, 4] == 255 and img_util.mip_to_uint8(flat_but_one)[0, 0] == 0
    assert img_util.mip_to_uint8(planes[0]).max() == 255 and img_util.mip_to_uint8(planes[0]).min() == 0


def test_compare_arguments_are_checked_before_a_device_is_needed():
    from aind_exaspim_image_compression import evaluate
    assert evaluate.abs_error_percentile is store_compare.abs_error_percentile
    a = np.zeros((4, 4, 4), np.uint16)
    for kw in (dict(window_size=0), dict(window_size=33), dict(data_range=0.0)):
        with pytest.raises(ValueError):
            evaluate.compare_volumes(a, a, **kw)
    with pytest.raises(ValueError):
        evaluate.compare_volumes(a, a.astype(np.float32))
    with pytest.raises(ValueError):
        evaluate.compare_volumes(a, a[:3])
    with pytest.raises(ValueError):
        evaluate.compare_stores("nowhere", "nowhere", budget_bytes=0)
