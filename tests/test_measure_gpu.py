"""Measuring a store on the MI355X: ``exabm4d_measure_box_u16_dev`` in guarded buffers against the
numpy restatement -- single boxes in windows of every alignment, a partition with odd corners against the whole-volume
kernels it replaces, data that stresses the tables kept in LDS, masks, the geometry checks -- and
``noise.measure_store`` against ``measure_volume`` and the in-memory estimators, for brick plans of many bricks and of
one."""
import numpy as np
import pytest

import measure_pyref as ref
from util import GuardedView

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.machine_learning import transforms
from aind_exaspim_image_compression.utils import chunk_store, noise, store_measure

pytestmark = pytest.mark.gpu
U16 = np.uint16
NOISE_WORDS = ref.LEVELS * ref.WIDE_BINS + ref.LEVELS
_CACHE = {}


def _octaves():
    if "octaves" not in _CACHE:
        vol = ref.octave_volume()
        mask = (vol > 330).astype(U16) * 3
        mask[4:6, 6:8, 8:10] = 0
        mask[5, 7, 9] = 1                                 # one voxel: the far corner of the cell at (4, 6, 8)
        for v in (vol, mask):
            v.setflags(write=False)
        _CACHE["octaves"] = (vol, mask, ref.box_tables(vol), ref.box_tables(vol, mask=mask))
    return _CACHE["octaves"]


def _window(vol, origin, dims):
    """The window ``origin + [0, dims)`` of ``vol``; what lies past the volume's faces holds 65535."""
    out = np.full(dims, 65535, dtype=U16)
    inside = tuple(slice(0, min(d, n - o)) for o, d, n in zip(origin, dims, vol.shape))
    out[inside] = vol[tuple(slice(o, o + s.stop) for o, s in zip(origin, inside))]
    return out


def _flat(tables):
    """(counts, noise) as the device lays them out, from the pyref's (counts, wide, sum_s)."""
    counts, wide, sum_s = tables
    noise_words = np.concatenate([wide.reshape(-1, ref.LEVELS * ref.WIDE_BINS), sum_s.reshape(-1, ref.LEVELS)], axis=1)
    return counts.reshape(-1), noise_words.reshape(-1)


def _measure(ctx, vol, mask, calls, k=0, mask_k=None, what=""):
    """Runs ``calls`` = [(w0, wd, b0, bd)] into guarded, poisoned tables (the first call zeroes them), each from its own
    guarded windows at element offset ``k``; checks the tables and their surroundings after every call against the sum
    of the pyref's boxes; returns the final (counts, noise)."""
    tables = 2 if mask is not None else 1
    counts = GuardedView(ctx, np.uint64, tables * ref.COUNT_BINS)
    noise_tab = GuardedView(ctx, np.uint64, tables * NOISE_WORDS)
    want = None
    try:
        for i, (w0, wd, b0, bd) in enumerate(calls):
            n = int(np.prod(wd))
            win = GuardedView(ctx, U16, n, k=k, data=_window(vol, w0, wd))
            mwin = None
            try:
                if mask is not None:
                    mwin = GuardedView(ctx, U16, n, k=k if mask_k is None else mask_k, data=_window(mask, w0, wd))
                ctx.measure_box_u16(win.ptr, mwin.ptr if mwin else None, vol.shape, w0, wd, b0, bd, counts.ptr,
                                    noise_tab.ptr, zero_first=i == 0)
                part = _flat(ref.box_tables(vol, b0, bd, mask))
                want = part if want is None else tuple(a + b for a, b in zip(want, part))
                ctx.sync()
                counts.check_output(want[0], f"{what} call {i}: counts")
                noise_tab.check_output(want[1], f"{what} call {i}: noise")
                win.check_untouched(f"{what} call {i}: window")
            finally:
                win.free()
                if mwin:
                    mwin.free()
        return want
    finally:
        counts.free()
        noise_tab.free()


# ---- the entry against the pyref: one box ---------------------------------------------------------------------------
# (window origin, window dims, box origin, box dims, element offset of the device pointer).  The volume is 22 x 19 x 27.
SINGLE = {
    "whole, pitch 27 (element loads)": ((0, 0, 0), (22, 19, 27), (0, 0, 0), (22, 19, 27), 0),
    "window past the x face, pitch 32 (vector loads)": ((0, 0, 0), (22, 19, 32), (0, 0, 0), (22, 19, 27), 0),
    "window at (2, 1, 2), pitch 24 (vector loads from x = 2)": ((2, 1, 2), (20, 18, 24), (3, 2, 5), (17, 15, 19), 0),
    "the same, pointer + 1 element (odd phase: element loads)": ((2, 1, 2), (20, 18, 24), (3, 2, 5), (17, 15, 19), 1),
    "window at odd x = 3, pointer + 1 (vector loads from x = 2 + 8 i)": ((1, 0, 3), (21, 19, 24), (2, 1, 3), (19, 17, 23), 1),
    "pitch 25 breaks the alignment": ((0, 0, 2), (22, 19, 25), (1, 1, 2), (20, 18, 25), 0),
    "pointer + 3 elements, window at x = 1 (vector loads from x = 6)": ((0, 0, 1), (22, 19, 24), (0, 0, 1), (22, 19, 23), 3),
}


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_box(ctx, case, with_mask):
    vol, mask, _, _ = _octaves()
    w0, wd, b0, bd, k = SINGLE[case]
    got = _measure(ctx, vol, mask if with_mask else None, [(w0, wd, b0, bd)], k=k, what=case)
    assert int(got[0].sum()) == int(np.prod(bd))


def test_box_equal_to_the_volume_is_the_whole_volume_kernels(ctx):
    vol, mask, whole, _ = _octaves()
    got = _measure(ctx, vol, None, [((0, 0, 0), vol.shape, (0, 0, 0), vol.shape)], what="whole")
    np.testing.assert_array_equal(got[0], _flat(whole)[0])
    np.testing.assert_array_equal(got[1], _flat(whole)[1])
    # a mask at another phase of 16 bytes than the window: element loads for both
    _measure(ctx, vol, mask, [((0, 0, 0), (22, 19, 32), (0, 0, 0), vol.shape)], k=0, mask_k=2, what="mask phase")


# ---- a partition with odd corners -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
def test_partition(ctx, with_mask):
    vol, mask, whole, whole_masked = _octaves()
    boxes = ref.partition(vol.shape, ([7, 8], [9], [5, 13]))
    assert len(boxes) == 18 and ((7, 0, 0), (1, 9, 5)) in boxes        # one voxel thick, inside the cell layer (6, 7)
    calls = []
    for b0, bd in boxes:
        win = [store_measure.cell_window(o, e, n) for o, e, n in zip(b0, bd, vol.shape)]
        calls.append((tuple(w[0] for w in win), tuple(w[1] for w in win), b0, bd))
    assert any(c[1] != c[3] for c in calls)                            # some windows hold a far corner outside their box
    counts, noise_words = _measure(ctx, vol, mask if with_mask else None, calls, what="partition")
    want = _flat(whole_masked if with_mask else whole)
    np.testing.assert_array_equal(counts, want[0])
    np.testing.assert_array_equal(noise_words, want[1])
    if with_mask:
        counts = counts.reshape(2, -1).sum(axis=0)
        noise_words = noise_words.reshape(2, -1).sum(axis=0)
    # the kernels it replaces, on the whole volume
    buf = ctx.to_device(vol)
    try:
        np.testing.assert_array_equal(counts, ctx.u16_histogram(buf, vol.size))
        wide = noise_words[:ref.LEVELS * ref.WIDE_BINS].reshape(ref.LEVELS, ref.WIDE_BINS)
        for k in range(7):
            hist, sum_s, skipped = ctx.noise_table(buf, U16, vol.shape, k)
            np.testing.assert_array_equal(store_measure.fold_noise_table(wide, k), hist, err_msg=f"shift {k}")
            np.testing.assert_array_equal(noise_words[ref.LEVELS * ref.WIDE_BINS:], sum_s)
            assert skipped == 0
    finally:
        buf.free()


# ---- the tables kept in LDS -------------------------------------------------------------------------------------------------
def _stress(kind):
    shape = (22, 19, 27)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    if kind == "constant":
        return np.full(shape, 321, dtype=U16)
    if kind == "constant beyond the band":
        return np.full(shape, 40000, dtype=U16)
    if kind == "checkerboard":
        return (((z + y + x) & 1) * 65535).astype(U16)
    if kind == "levels":
        # a cell layer per value: eleven levels at once, more than the slots, so some rows take the global path
        values = np.array([0, 20, 40, 80, 160, 320, 640, 1280, 2560, 5120, 10240])
        rng = np.random.default_rng(11)
        return (values[z // 2] + rng.integers(0, 8, shape)).astype(U16)
    if kind == "long rows":
        rng = np.random.default_rng(12)
        return rng.integers(0, 65536, (3, 5, 8301)).astype(U16)        # more groups of eight than lanes; every value
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["constant", "constant beyond the band", "checkerboard", "levels", "long rows"])
def test_privatisation(ctx, kind):
    vol = _stress(kind)
    counts, wide, sum_s = ref.box_tables(vol)
    levels = np.nonzero(wide.sum(axis=1))[0]
    if kind.startswith("constant"):
        assert levels.size == 1 and np.count_nonzero(wide) == 1 and wide[levels[0], 0] == 11 * 9 * 13   # one bin
        assert np.count_nonzero(counts) == 1
    if kind == "checkerboard":
        assert wide[:, ref.WIDE_BINS - 1].sum() == wide.sum() > 0              # every cell in the highest wide bin
        assert counts[0] > 0 and counts[65535] > 0
        zeros = np.zeros_like(vol)
        zeros[:2] = 65535                                                      # ... and both extreme levels
        both = np.concatenate([zeros, vol], axis=0)
        lv = np.nonzero(ref.box_tables(both)[1].sum(axis=1))[0]
        assert lv[0] == 0 and lv[-1] == ref.LEVELS - 1
        _measure(ctx, both, None, [((0, 0, 0), both.shape, (0, 0, 0), both.shape)], what="extreme levels")
    if kind == "levels":
        assert levels.size > 8
    _measure(ctx, vol, None, [((0, 0, 0), vol.shape, (0, 0, 0), vol.shape)], what=kind)
    if kind == "levels":
        mask = (vol % 3 == 0).astype(U16)
        _measure(ctx, vol, mask, [((0, 0, 0), vol.shape, (0, 0, 0), vol.shape)], what=kind + " masked")


# ---- masks --------------------------------------------------------------------------------------------------------------------
def test_mask(ctx):
    vol, mask, whole, whole_masked = _octaves()
    geometry = ((0, 0, 0), vol.shape, (0, 0, 0), vol.shape)
    counts, noise_words = _measure(ctx, vol, mask, [geometry], what="mask")          # classification against the pyref
    plain = _flat(whole)
    np.testing.assert_array_equal(counts.reshape(2, -1).sum(axis=0), plain[0])       # fg + bg = unmasked
    np.testing.assert_array_equal(noise_words.reshape(2, -1).sum(axis=0), plain[1])
    # the mask touches exactly one voxel of the cell at (4, 6, 8), its far corner: the cell is foreground
    assert np.count_nonzero(mask[4:6, 6:8, 8:10]) == 1 and mask[5, 7, 9]
    s, m, _ = ref.npr.cell_values(vol[4:6, 6:8, 8:10])
    fg_wide = whole_masked[1][0]
    assert fg_wide[ref.npr.level_of(s)[0], ref.wide_bin(m)[0]] >= 1
    without = mask.copy()
    without[5, 7, 9] = 0
    assert ref.box_tables(vol, mask=without)[1][0].sum() == fg_wide.sum() - 1
    # no mask at all is the background of a mask of zeros
    zeros = np.zeros_like(mask)
    counts0, noise0 = _measure(ctx, vol, zeros, [geometry], what="zero mask")
    assert not counts0.reshape(2, -1)[0].any() and not noise0.reshape(2, -1)[0].any()
    np.testing.assert_array_equal(counts0.reshape(2, -1)[1], plain[0])
    np.testing.assert_array_equal(noise0.reshape(2, -1)[1], plain[1])


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_geometry_is_checked_on_the_host(ctx):
    vol, _, _, _ = _octaves()
    w0, wd = (2, 1, 2), (20, 18, 24)
    win = GuardedView(ctx, U16, int(np.prod(wd)), data=_window(vol, w0, wd))
    counts = GuardedView(ctx, np.uint64, ref.COUNT_BINS)
    noise_tab = GuardedView(ctx, np.uint64, NOISE_WORDS)
    good = dict(vol=vol.shape, w0=w0, wd=wd, b0=(3, 2, 5), bd=(17, 15, 19))
    try:
        # the window holds z 2..21, y 1..18, x 2..25.  Boxes whose last cells end with the window are accepted:
        fine = [dict(bd=(19, 15, 19)),          # the cell layer z = 20 needs z = 21, the window's (and the volume's) last
                dict(bd=(17, 15, 21))]          # the cell at x = 24 needs x = 25, the window's last
        for case in fine:
            g = {**good, **case}
            ctx.measure_box_u16(win.ptr, None, *g.values(), counts.ptr, noise_tab.ptr, zero_first=True)
            ctx.sync()
            want = _flat(ref.box_tables(vol, g["b0"], g["bd"]))
            counts.check_output(want[0], "a box that ends with its window: counts")
            noise_tab.check_output(want[1], "a box that ends with its window: noise")
        fresh = [GuardedView(ctx, np.uint64, ref.COUNT_BINS), GuardedView(ctx, np.uint64, NOISE_WORDS)]
        try:
            missing = [dict(bd=(17, 15, 20), wd=(20, 18, 23)),       # the cell at x = 24 needs x = 25, the window ends at 24
                       dict(wd=(20, 16, 24)),                        # the cell row y = 16 needs y = 17, the window ends at 16
                       dict(bd=(18, 15, 19), wd=(19, 18, 24))]       # the cell layer z = 20 needs z = 21, ... at 20
            for case in missing:
                with pytest.raises(ValueError, match="far corner"):
                    ctx.measure_box_u16(win.ptr, None, *{**good, **case}.values(), fresh[0].ptr, fresh[1].ptr,
                                        zero_first=True)
            outside = [dict(b0=(1, 2, 5)), dict(bd=(17, 15, 22)), dict(bd=(17, 0, 19)), dict(w0=(-1, 1, 2)),
                       dict(vol=(22, 19, 20)), dict(wd=(20, 18, 0))]
            for case in outside:
                with pytest.raises(ValueError):
                    ctx.measure_box_u16(win.ptr, None, *{**good, **case}.values(), fresh[0].ptr, fresh[1].ptr,
                                        zero_first=True)
            for c, n in ((None, fresh[1].ptr), (fresh[0].ptr, None)):
                with pytest.raises(ValueError):
                    ctx.measure_box_u16(win.ptr, None, *good.values(), c, n, zero_first=True)
            with pytest.raises(ValueError):
                ctx.measure_box_u16(None, None, *good.values(), fresh[0].ptr, fresh[1].ptr, zero_first=True)
            ctx.sync()
            for f in fresh:
                f.check_untouched("a rejected measure_box")          # not even zeroed: nothing was launched
        finally:
            for f in fresh:
                f.free()
        # a valid call afterwards works
        ctx.measure_box_u16(win.ptr, None, *good.values(), counts.ptr, noise_tab.ptr, zero_first=True)
        ctx.sync()
        want = _flat(ref.box_tables(vol, good["b0"], good["bd"]))
        counts.check_output(want[0], "after rejected calls: counts")
        noise_tab.check_output(want[1], "after rejected calls: noise")
    finally:
        for v in (win, counts, noise_tab):
            v.free()


# ---- noise.measure_store ------------------------------------------------------------------------------------------------------------
SHAPE = (40, 36, 44)
BRICKED, WHOLE = 20_000, 1 << 30


def _store_volume(kind):
    rng = np.random.default_rng(21)
    z, y, x = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    if kind == "quiet":
        # a Poisson-Gaussian ramp: gain 2, read noise 5, offset 100
        clean = 40.0 * np.exp(x / 12.0)
        vol = 100.0 + 2.0 * rng.poisson(clean / 2.0) + rng.normal(0.0, 5.0, SHAPE)
    else:
        # noise so large that the table saturates at the small shifts
        vol = 30000.0 + rng.normal(0.0, 9000.0, SHAPE)
    vol = np.rint(np.clip(vol, 0, 65535)).astype(U16)
    vol[:, :2, :3] = 0                                     # zeros, which the offset ignores
    return vol


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    base = tmp_path_factory.mktemp("measure-stores")
    out = {}
    for kind in ("quiet", "loud"):
        vol = _store_volume(kind)
        mask = (vol > np.percentile(vol, 80)).astype(U16)
        paths = {}
        for name, chunks in (("even", (16, 16, 16)), ("odd", (15, 13, 17))):
            paths[name] = str(base / f"{kind}-{name}")
            chunk_store.write_zarr(vol, paths[name], (1, 1) + chunks)
            np.testing.assert_array_equal(chunk_store.read_zarr(paths[name])[0, 0], vol)
        paths["mask"] = str(base / f"{kind}-mask")
        chunk_store.write_zarr(mask, paths["mask"], (1, 1, 16, 16, 16))
        vol.setflags(write=False)
        out[kind] = (paths, vol, mask, noise.measure_volume(vol), noise.measure_volume(vol, mask))
    return out


def _same(got, want, what):
    assert got.shape == want.shape and got.masked == want.masked, what
    for f in ("counts", "noise_wide", "sum_s") + (("counts_fg", "counts_bg", "noise_wide_fg", "noise_wide_bg", "sum_s_fg",
                                                   "sum_s_bg") if want.masked else ()):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == np.uint64 and a.shape == b.shape, (what, f)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {f}")


def test_measure_volume_is_the_pyref(stores):
    for kind, (_, vol, mask, whole, masked) in stores.items():
        for m, tables in ((whole, ref.box_tables(vol)), (masked, ref.box_tables(vol, mask=mask))):
            counts, wide, sum_s = tables
            if m.masked:
                np.testing.assert_array_equal(np.stack([m.counts_fg, m.counts_bg]), counts)
                np.testing.assert_array_equal(np.stack([m.noise_wide_fg, m.noise_wide_bg]), wide)
                np.testing.assert_array_equal(np.stack([m.sum_s_fg, m.sum_s_bg]), sum_s)
                counts, wide, sum_s = counts.sum(axis=0), wide.sum(axis=0), sum_s.sum(axis=0)
            np.testing.assert_array_equal(m.counts, counts, err_msg=kind)
            np.testing.assert_array_equal(m.noise_wide, wide, err_msg=kind)
            np.testing.assert_array_equal(m.sum_s, sum_s, err_msg=kind)


@pytest.mark.parametrize("chunks", ["even", "odd"])
@pytest.mark.parametrize("kind", ["quiet", "loud"])
def test_measure_store(stores, kind, chunks):
    paths, vol, mask, whole, masked = stores[kind]
    n = vol.size
    chunk = (16, 16, 16) if chunks == "even" else (15, 13, 17)
    plan = store_measure.plan_measure(SHAPE, chunk, BRICKED)
    assert len(plan) >= 8 and all(len({br.origin[ax] for br in plan}) >= 2 for ax in range(3))
    stats = {}
    got = noise.measure_store(paths[chunks], budget_bytes=BRICKED, stats=stats)
    _same(got, whole, f"{kind} {chunks} bricked")
    assert stats["bricks"] == len(plan) and stats["passes"] == 1
    # every brick is read once, with at most a voxel more per axis
    assert n <= stats["voxels_read"] == sum(br.window_voxels for br in plan)
    assert stats["voxels_read"] <= sum(int(np.prod([e + 1 for e in br.extent])) for br in plan) < n + n // 2
    assert set(stats["seconds"]) == {"read", "measure", "download"}
    assert stats["largest_alloc"] >= 2 * max(br.window_voxels for br in plan)
    one_stats = {}
    one = noise.measure_store(chunk_store.open_zarr(paths[chunks]), budget_bytes=WHOLE, stats=one_stats)
    _same(one, whole, f"{kind} {chunks} one brick")
    assert one_stats["bricks"] == 1 and one_stats["voxels_read"] == n and one_stats["passes"] == 1
    # with a mask store (chunks of its own)
    _same(noise.measure_store(paths[chunks], mask=paths["mask"], budget_bytes=BRICKED), masked, f"{kind} {chunks} masked")

    # the estimators, bit for bit those of the array in memory
    assert got.n == n and got.min == int(vol.min()) and got.max == int(vol.max())
    for p in (1.0, 0.1):
        assert got.offset(p) == transforms.estimate_offset(vol, p)
    assert got.offset(1.0, ignore_zeros=False) == transforms.estimate_offset(vol, 1.0, ignore_zeros=False)
    assert got.background_offset_statistics() == transforms.background_offset_statistics(vol)
    assert got.background_offset_statistics(1.0) == transforms.background_offset_statistics(vol, 1.0)
    for min_cells in (512, 64):
        want = noise.noise_table(vol, min_cells=min_cells)
        table = got.noise_table(min_cells=min_cells)
        assert table.shift == want.shift and table.skipped == want.skipped == 0
        np.testing.assert_array_equal(table.hist, want.hist)
        np.testing.assert_array_equal(table.sum_s, want.sum_s)
        for a, b in zip(got.noise_curve(min_cells), noise.noise_curve(vol, min_cells)):
            np.testing.assert_array_equal(a, b)
    assert got.sigma() == noise.estimate_sigma(vol) > 0.0
    if kind == "loud":
        # the in-memory rule repeats its pass twice or more; the store was read once all the same
        assert noise.noise_table(vol).shift >= 2 and stats["passes"] == 1 and stats["voxels_read"] < n + n // 2
    else:
        assert noise.noise_table(vol).shift == 0
        # (7920 cells over a dozen levels: fewer than the default 512 a level)
        pg = got.poisson_gaussian(min_cells=128)
        assert pg == noise.estimate_poisson_gaussian(vol, min_cells=128)
        assert pg == noise.estimate_poisson_gaussian(vol, offset=got.offset(), min_cells=128)
        assert got.poisson_gaussian(offset=90.0, min_cells=64) == noise.estimate_poisson_gaussian(vol, 90.0, 64)
        assert got.anscombe_cfg(min_cells=128) == noise.anscombe_cfg(vol, min_cells=128)
        assert 1.0 < pg["gain"] < 4.0                                      # the data was made with gain 2

    base = transforms.build_transform({"kind": "asinh", "params": {"offset": 0.0, "scale": 40.0, "max_count": 4000.0}})
    for p in (0.1, 1.0):
        a = inference.build_volume_transform(base, img=got, percentile=p)
        b = inference.build_volume_transform(base, img=vol, percentile=p)
        assert a.cfg == b.cfg and a.cfg["kind"] == "offset" and a.cfg["params"]["offset"] == got.offset(p)


def test_measure_arguments(stores):
    paths = stores["quiet"][0]
    with pytest.raises(ValueError):
        noise.measure_store(paths["even"], budget_bytes=0)
    with pytest.raises(ValueError):
        noise.measure_volume(np.zeros((4, 4, 4), np.float32))
    with pytest.raises(ValueError):
        noise.measure_volume(np.zeros((4, 4), U16))
    with pytest.raises(ValueError):
        noise.measure_volume(np.zeros((4, 4, 4), U16), mask=np.zeros((4, 4, 5), U16))
    tiny = noise.measure_volume(np.full((1, 3, 2), 7, U16))                # no cell at all: the counts alone
    assert tiny.n == 6 and tiny.counts[7] == 6 and not tiny.noise_wide.any()
