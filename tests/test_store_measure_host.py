"""The host side of measuring a store, without a device: the wide noise table folds into the table
of every shift exactly, the brick plan partitions the volume and every brick's window holds the cells it owns, the
ownership rule adds up over any partition, and the estimators of ``StoreMeasure`` on numpy-built tables equal the numpy
restatements of the in-memory ones."""
import math

import numpy as np
import pytest

import measure_pyref as ref
import noise_pyref as npr

from aind_exaspim_image_compression.utils import store_measure
from aind_exaspim_image_compression.utils.store_measure import StoreMeasure

U16 = np.uint16


def _random_volume(shape=(20, 18, 26), seed=2, sigma=30.0):
    rng = np.random.default_rng(seed)
    ramp = np.linspace(100.0, 1200.0, shape[2])[None, None, :]
    return np.rint(np.clip(ramp + rng.normal(0.0, sigma, shape) * np.sqrt(ramp / 100.0), 0, 65535)).astype(U16)


def _measure_of(vol, mask=None):
    counts, wide, sum_s = ref.box_tables(vol, mask=mask)
    noise = np.concatenate([wide.reshape(-1, ref.LEVELS * ref.WIDE_BINS), sum_s.reshape(-1, ref.LEVELS)], axis=1)
    return StoreMeasure.from_tables(vol.shape, counts, noise)


# ---- the wide table -------------------------------------------------------------------------------------------------
def test_every_m_folds_into_its_bin_at_every_shift():
    m = np.arange(ref.M_MAX + 1)
    w = store_measure.wide_bin(m)
    np.testing.assert_array_equal(w, ref.wide_bin(m))
    assert w.min() == 0 and w.max() == store_measure.WIDE_BINS - 1 == 16383
    assert np.all(np.diff(w) >= 0) and np.unique(w).size == 16384
    v0 = store_measure.wide_low_value(np.arange(16384))
    np.testing.assert_array_equal(v0, ref.wide_low_values())
    for k in range(7):
        np.testing.assert_array_equal(np.minimum(v0[w] >> k, 4095), np.minimum(m >> k, 4095), err_msg=f"shift {k}")
    assert int(store_measure.wide_bin(4095)) == 4095 and int(store_measure.wide_bin(4096)) == 4096
    assert int(store_measure.wide_bin(ref.M_MAX)) == 16383
    for bad in (-1, ref.M_MAX + 1):
        with pytest.raises(ValueError):
            store_measure.wide_bin(bad)
    with pytest.raises(ValueError):
        store_measure.wide_low_value(16384)


@pytest.mark.parametrize("kind", ["random", "octaves"])
def test_fold_equals_the_table_of_every_shift(kind):
    vol = _random_volume() if kind == "random" else ref.octave_volume()
    counts, wide, sum_s = ref.box_tables(vol)
    assert wide.sum() == np.prod([n // 2 for n in vol.shape])
    if kind == "octaves":
        assert vol.shape == (22, 19, 27)
        per_bin = wide.sum(axis=0)
        for j in range(1, 7):                            # every octave of the wide table is hit
            assert per_bin[4096 + (j - 1) * 2048:4096 + j * 2048].sum() > 0, j
        assert per_bin[16383] >= 1                       # |d| = 4 * 65535
        _, m, _ = npr.cell_values(vol)
        assert m.max() == ref.M_MAX
    for k in range(7):
        hist, want_s, _ = npr.table(vol, k)
        got = store_measure.fold_noise_table(wide, k)
        assert got.dtype == np.uint64 and got.shape == (npr.LEVELS, npr.BINS)
        np.testing.assert_array_equal(got, hist, err_msg=f"shift {k}")
        np.testing.assert_array_equal(ref.fold(wide, k), hist, err_msg=f"pyref fold, shift {k}")
        np.testing.assert_array_equal(sum_s, want_s)
    np.testing.assert_array_equal(counts, np.bincount(vol.reshape(-1), minlength=65536))
    with pytest.raises(ValueError):
        store_measure.fold_noise_table(wide, 7)
    with pytest.raises(ValueError):
        store_measure.fold_noise_table(wide[:, :4096], 0)


def test_the_auto_rule_needs_a_larger_shift_on_the_octave_volume():
    """The case the wide table is for: in memory the rule repeats its pass, here it folds again."""
    vol = ref.octave_volume()
    shift = npr.auto_table(vol, min_cells=64)[3]
    assert shift >= 2
    assert _measure_of(vol).noise_table(min_cells=64).shift == shift


# ---- the brick plan -------------------------------------------------------------------------------------------------
PLANS = [((40, 36, 44), (16, 16, 16), 20_000), ((40, 36, 44), (16, 16, 16), 60_000), ((40, 36, 44), (15, 13, 17), 60_000),
         ((40, 36, 44), (15, 13, 17), 1),
         ((41, 37, 45), (16, 16, 16), 150_000), ((40, 36, 44), (64, 64, 64), 1 << 30), ((23, 9, 31), (8, 9, 7), 30_000),
         ((40, 36, 44), (16, 16, 16), 1 << 30), ((7, 1, 5), (3, 1, 2), 1 << 20)]


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("shape,chunk,budget", PLANS)
def test_plan_measure(shape, chunk, budget, with_mask):
    bricks = store_measure.plan_measure(shape, chunk, budget, with_mask)
    seen = np.zeros(shape, dtype=np.int32)
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    for br in bricks:
        seen[tuple(slice(o, o + e) for o, e in zip(br.origin, br.extent))] += 1
        in_chunks = []
        for a in range(3):
            o, e, w0, wn = br.origin[a], br.extent[a], br.win_origin[a], br.win_extent[a]
            assert o % chunk[a] == 0 and (e % chunk[a] == 0 or o + e == shape[a])        # whole chunks
            in_chunks.append(-(-e // chunk[a]))
            # the window: the brick, extended to the next even coordinate, cut at the face
            end = o + e
            assert w0 == o and w0 + wn == min(end + end % 2, shape[a])
            # every cell the brick owns (even origin in the brick, below dim & ~1) has its far corner in the window
            owned = [c for c in range(o + o % 2, end, 2) if c < shape[a] - shape[a] % 2]
            assert all(w0 <= c and c + 1 < w0 + wn for c in owned)
        slabs = -(-br.win_extent[0] // chunk[0])
        held = slabs * -(-br.win_extent[0] // slabs) * br.win_extent[1] * br.win_extent[2]
        stores = 2 if with_mask else 1
        assert br.cost == stores * (2 * held + budget // 8)
        assert br.cost <= budget or in_chunks == [1, 1, 1]
    assert np.all(seen == 1)                                                           # a partition
    assert [br.origin for br in bricks] == sorted(br.origin for br in bricks)          # raster order
    if budget >= 1 << 30:
        assert len(bricks) == 1 and bricks[0].extent == shape == bricks[0].win_extent
    if budget == 1:
        assert len(bricks) == grid[0] * grid[1] * grid[2]


def test_plan_measure_arguments():
    assert len(store_measure.plan_measure((40, 36, 44), (16, 16, 16), 20_000)) >= 8
    for bad in (((40, 36), (16, 16, 16), 1), ((40, 36, 0), (16, 16, 16), 1), ((40, 36, 44), (16, 0, 16), 1),
                ((40, 36, 44), (16, 16, 16), 0)):
        with pytest.raises(ValueError):
            store_measure.plan_measure(*bad)


# ---- ownership --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
def test_a_partition_with_odd_corners_adds_up_to_the_volume(with_mask):
    vol = ref.octave_volume()
    mask = (vol > 330).astype(U16) if with_mask else None
    boxes = ref.partition(vol.shape, ([7, 8], [9], [5, 13]))
    assert len(boxes) == 18 and ((7, 0, 0), (1, 9, 5)) in boxes
    total = None
    for b0, bd in boxes:
        part = ref.box_tables(vol, b0, bd, mask)
        total = part if total is None else tuple(t + p for t, p in zip(total, part))
    for got, want in zip(total, ref.box_tables(vol, mask=mask)):
        np.testing.assert_array_equal(got, want)
    if with_mask:
        for both, one in zip(total, ref.box_tables(vol)):
            np.testing.assert_array_equal(both[0] + both[1], one)
    # the thin box z = 7 lies inside the cell layer (6, 7): it owns voxels and no cell
    counts, wide, _ = ref.box_tables(vol, (7, 0, 0), (1, 9, 5))
    assert counts.sum() == 45 and wide.sum() == 0


# ---- the estimators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "octaves", "zeros"])
def test_estimators_equal_the_numpy_restatements(kind):
    vol = {"random": _random_volume, "octaves": ref.octave_volume}.get(kind, _random_volume)()
    if kind == "zeros":
        vol = vol.copy()
        vol[:, :5] = 0
    m = _measure_of(vol)
    assert m.shape == vol.shape and m.n == vol.size and not m.masked
    assert m.min == int(vol.min()) and m.max == int(vol.max())
    assert m.zero_fraction == 1.0 - np.count_nonzero(vol) / vol.size
    x32 = vol.astype(np.float32).reshape(-1)
    for p in (1.0, 0.1, 50.0):
        assert m.offset(p) == float(np.percentile(x32[x32 > 0], p))
        assert m.offset(p, ignore_zeros=False) == float(np.percentile(x32, p))
    flat = vol.reshape(-1)
    stats = m.background_offset_statistics(0.1)
    assert stats["offset"] == float(np.percentile(flat[flat > 0], 0.1))
    assert stats["offset_all_voxels"] == float(np.percentile(flat, 0.1))
    assert stats["median"] == float(np.median(flat[flat > 0]))
    assert stats["zero_fraction"] == m.zero_fraction
    for min_cells in (512, 40):
        hist, sum_s, _, shift = npr.auto_table(vol, min_cells)
        table = m.noise_table(min_cells=min_cells)
        assert table.shift == shift and table.skipped == 0
        np.testing.assert_array_equal(table.hist, hist)
        np.testing.assert_array_equal(table.sum_s, sum_s)
        want = npr.noise_curve(vol, min_cells)
        got = m.noise_curve(min_cells)
        assert len(want[0]) >= (3 if min_cells == 40 else 0)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        if len(want[0]) >= 3:
            try:
                want_pg = npr.estimate_poisson_gaussian(vol, 37.5, min_cells)
            except ValueError:
                with pytest.raises(ValueError):
                    m.poisson_gaussian(37.5, min_cells)
            else:
                assert m.poisson_gaussian(37.5, min_cells) == want_pg
                assert m.poisson_gaussian(min_cells=min_cells) == npr.estimate_poisson_gaussian(vol, m.offset(), min_cells)
                assert m.anscombe_cfg(min_cells=min_cells) == {"kind": "anscombe",
                                                               "params": m.poisson_gaussian(min_cells=min_cells)}
    sigma = m.sigma()
    assert sigma == npr.estimate_sigma(vol) and math.isfinite(sigma) and sigma > 0.0
    k = 3
    np.testing.assert_array_equal(m.noise_table(shift=k).hist, npr.table(vol, k)[0])
    with pytest.raises(ValueError):
        m.noise_table(which="bg")
    with pytest.raises(ValueError):
        m.noise_table(shift=7)


def test_a_masked_measurement_splits_and_adds_up():
    vol = _random_volume()
    mask = np.zeros(vol.shape, dtype=U16)
    mask[:, :, 14:] = 9
    mask[5, 7, 9] = 1                       # one voxel, the far corner of the cell at (4, 6, 8)
    m = _measure_of(vol, mask)
    plain = _measure_of(vol)
    assert m.masked
    np.testing.assert_array_equal(m.counts, plain.counts)
    np.testing.assert_array_equal(m.noise_wide, plain.noise_wide)
    np.testing.assert_array_equal(m.sum_s, plain.sum_s)
    assert int(m.counts_fg.sum()) == int(np.count_nonzero(mask)) and int(m.counts_bg.sum()) == int((mask == 0).sum())
    cells = vol.size // 8
    assert int(m.noise_wide_fg.sum()) == 10 * 9 * 6 + 1 and int(m.noise_wide_bg.sum()) == cells - 10 * 9 * 6 - 1
    np.testing.assert_array_equal(m.noise_table(shift=0, which="bg").hist, npr.table(vol[:, :, :14], 0)[0] -
                                  m.noise_table(shift=0, which="fg").hist + npr.table(vol[:, :, 14:], 0)[0])
    assert m.sigma(which="bg") > 0.0 and m.sigma(which="fg") > m.sigma(which="bg")
    with pytest.raises(ValueError):
        m.noise_table(which="both")
    with pytest.raises(ValueError):
        StoreMeasure((3, 3, 3), plain.counts, plain.noise_wide, plain.sum_s)     # the counts are another volume's
