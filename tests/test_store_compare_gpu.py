"""Scoring one store against another on the MI355X: the three box kernels
(``exabm4d_diff_histogram_u16_dev``, ``exabm4d_mip3_u16_dev``, ``exabm4d_ssim3d_box_dev``) in guarded buffers against
numpy and the whole-volume SSIM entry, and ``evaluate.compare_stores`` against ``compare_volumes``, the in-memory
metric functions and numpy, for brick plans of many bricks and of one."""
import math

import numpy as np
import pytest

import compare_pyref as ref
from util import GuardedView

from aind_exaspim_image_compression import _native, evaluate
from aind_exaspim_image_compression.utils import chunk_store, img_util, store_compare
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec

pytestmark = pytest.mark.gpu
U16 = np.uint16
VOL = (37, 20, 70)
# (window origin, window dims, [boxes]): a window with non-zero origins on all axes whose boxes touch the z and x faces
# (the second one the y face too) and share projection planes; and the volume as its own window with a box of 2 x 2 x 2
# projection tiles and several histogram steps
GEOMETRIES = [
    ((5, 2, 20), (32, 18, 50), [((9, 4, 27), (28, 12, 43)), ((6, 3, 21), (20, 17, 40))]),
    ((0, 0, 0), VOL, [((1, 1, 1), (36, 19, 69)), ((0, 0, 0), (37, 20, 64))]),
]
_PAIRS = {}


def _pair(kind, shape=VOL):
    key = (kind, shape)
    if key not in _PAIRS:
        a, b = ref.synth_pair(shape, seed=3) if kind == "synth" else ref.full_range_pair(shape, 4)
        mask = (a > np.percentile(a, 80)).astype(U16) * 7          # non-zero = foreground
        for v in (a, b, mask):
            v.setflags(write=False)
        _PAIRS[key] = (a, b, mask)
    return _PAIRS[key]


def _window(vol, origin, dims):
    return np.ascontiguousarray(vol[ref.box_slices(origin, dims)])


def _views(ctx, vols, origin, dims):
    """The windows of ``vols`` at an odd element offset (2-byte alignment only), guarded."""
    n = int(np.prod(dims))
    return [GuardedView(ctx, U16, n, k=1, data=_window(v, origin, dims)) for v in vols]


# ---- kernel a: exabm4d_diff_histogram_u16_dev ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["synth", "full_range"])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("geometry", [0, 1])
def test_diff_histogram(ctx, kind, with_mask, geometry):
    a, b, mask = _pair(kind)
    w0, wd, boxes = GEOMETRIES[geometry]
    tables = 2 if with_mask else 1
    wins = _views(ctx, (a, b, mask), w0, wd)
    hist = GuardedView(ctx, np.uint64, tables * ref.DIFF_BINS)        # poisoned: the first call zeroes it
    try:
        want = np.zeros((tables, ref.DIFF_BINS), np.uint64)
        for k, (b0, bd) in enumerate(boxes):
            ctx.diff_histogram_u16(wins[0].ptr, wins[1].ptr, wins[2].ptr if with_mask else None, VOL, w0, wd, b0, bd,
                                   hist.ptr, zero_first=k == 0)
            t = ref.diff_table(a, b, b0, bd, mask if with_mask else None)
            want += np.stack(t) if with_mask else t[None]
            ctx.sync()
            hist.check_output(want, f"diff_histogram {kind} mask={with_mask} box {k}")
        assert int(want.sum()) == sum(int(np.prod(bd)) for _, bd in boxes)
        if kind == "full_range" and geometry == 1:
            assert want.sum(axis=0)[0] >= 1 and want.sum(axis=0)[-1] >= 1     # the end bins: 0 - 65535 and 65535 - 0
        for w in wins:
            w.check_untouched("diff_histogram inputs")
    finally:
        for v in wins + [hist]:
            v.free()


# ---- kernel b: exabm4d_mip3_u16_dev ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["synth", "full_range"])
@pytest.mark.parametrize("geometry", [0, 1])
def test_mip3(ctx, kind, geometry):
    a, b, _ = _pair(kind)
    w0, wd, boxes = GEOMETRIES[geometry]
    words = 3 * _native.mip_plane_words(VOL)
    wins = _views(ctx, (a, b), w0, wd)
    planes = GuardedView(ctx, np.uint32, words, data=np.zeros(words, np.uint32))
    try:
        want = ref.empty_mips(VOL)
        for k, (b0, bd) in enumerate(boxes):
            ctx.mip3_u16(wins[0].ptr, wins[1].ptr, VOL, w0, wd, b0, bd, planes.ptr)
            ref.fold_mips(want, a, b, b0, bd)
            ctx.sync()
            flat = np.concatenate([p.reshape(-1) for name in ("ref", "test", "abs_diff") for p in want[name]])
            planes.check_output(flat.astype(np.uint32), f"mip3 {kind} box {k}")
        got = _native.split_mip_planes(planes.buf.download(planes.host.shape, np.uint8)[planes.lo:planes.hi]
                                       .view(np.uint32), VOL)
        for name in want:
            for axis in range(3):
                assert got[name][axis].dtype == U16
                np.testing.assert_array_equal(got[name][axis], want[name][axis])
        for w in wins:
            w.check_untouched("mip3 inputs")
    finally:
        for v in wins + [planes]:
            v.free()


def test_mip3_of_the_whole_volume_is_numpy_max(ctx):
    a, b, _ = _pair("synth")
    words = 3 * _native.mip_plane_words(VOL)
    wins = _views(ctx, (a, b), (0, 0, 0), VOL)
    planes = ctx.alloc(4 * words).zero()
    try:
        ctx.mip3_u16(wins[0].ptr, wins[1].ptr, VOL, (0, 0, 0), VOL, (0, 0, 0), VOL, planes)
        ctx.sync()
        got = _native.split_mip_planes(planes.download((words,), np.uint32), VOL)
        diff = np.abs(b.astype(np.int32) - a.astype(np.int32))
        for name, vol in (("ref", a), ("test", b), ("abs_diff", diff)):
            for axis in range(3):
                np.testing.assert_array_equal(got[name][axis], np.max(vol, axis=axis))
    finally:
        planes.free()
        for v in wins:
            v.free()


# ---- kernel c: exabm4d_ssim3d_box_dev ---------------------------------------------------------------------------------
L = 1000.0
C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
_WHOLE = {}


def _whole_ssim(ctx, shape, window):
    """``exabm4d_ssim3d_dev``'s sum on the pair of ``shape``, computed once."""
    key = (shape, window)
    if key not in _WHOLE:
        a, b, _ = _pair("synth", shape)
        d_a, d_b = ctx.to_device(a), ctx.to_device(b)
        try:
            _WHOLE[key] = ctx.ssim3d_sum(d_a, d_b, U16, shape, window, C1, C2)
        finally:
            d_a.free()
            d_b.free()
    return _WHOLE[key]


def _halves(n):
    cut = n // 2 + 1
    return [(0, cut), (cut, n - cut)]


@pytest.mark.parametrize("shape", [VOL, (10, 40, 70)])          # (10, 40, 70): z is reflected more than once at 16
@pytest.mark.parametrize("window", [16, 7])
def test_ssim3d_box(ctx, shape, window):
    a, b, _ = _pair("synth", shape)
    n = int(np.prod(shape))
    whole = _whole_ssim(ctx, shape, window)
    # one box equal to the volume: the whole-volume entry's launch, bit for bit
    wins = _views(ctx, (a, b), (0, 0, 0), shape)
    try:
        got = ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, shape, (0, 0, 0), shape, (0, 0, 0), shape, window, C1, C2)
        assert got == whole
        for w in wins:
            w.check_untouched("ssim3d_box inputs")
    finally:
        for v in wins:
            v.free()
    # eight boxes, each in the smallest window that holds its halo: the same n terms in another order
    total, parts = 0.0, 0
    for bz in _halves(shape[0]):
        for by in _halves(shape[1]):
            for bx in _halves(shape[2]):
                b0, bd = tuple(q[0] for q in (bz, by, bx)), tuple(q[1] for q in (bz, by, bx))
                rng = [store_compare.halo_range(o, d, s, window) for o, d, s in zip(b0, bd, shape)]
                w0, wd = tuple(r[0] for r in rng), tuple(r[1] for r in rng)
                wins = _views(ctx, (a, b), w0, wd)
                try:
                    total += ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, shape, w0, wd, b0, bd, window, C1, C2)
                    parts += 1
                finally:
                    for v in wins:
                        v.free()
    assert parts == 8
    print(f"ssim3d_box {shape} w={window}: whole {whole / n!r}, eight boxes {total / n!r}")
    assert abs(total / n - whole / n) <= 2 * n * 2.0 ** -53
    assert 0.0 < whole / n < 1.0


def test_box_geometry_is_checked_on_the_host(ctx):
    a, b, _ = _pair("synth")
    w0, wd = (5, 2, 20), (32, 18, 50)
    wins = _views(ctx, (a, b), w0, wd)
    hist = GuardedView(ctx, np.uint64, ref.DIFF_BINS)
    planes = GuardedView(ctx, np.uint32, 3 * _native.mip_plane_words(VOL))
    try:
        # the box (13, 10, 28) + (16, 8, 24) and its halo of 8 below / 7 above lie in the window: accepted
        good = dict(vol=VOL, w0=w0, wd=wd, b0=(13, 10, 28), bd=(16, 8, 24))
        ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, *good.values(), 16, C1, C2)
        bad_ssim = [dict(b0=(12, 10, 28)),                  # the halo begins a layer in front of the window
                    dict(b0=(13, 10, 27)),                  # ... a column in front of it
                    dict(b0=(13, 2, 28)),                   # y 2 - 8 < 0 reflects to 0 .. 5: rows 0, 1 are not in the window
                    dict(wd=(30, 18, 50))]                  # the halo ends at z = 35, the window at 34
        for case in bad_ssim:
            g = dict(good)
            g.update(case)
            with pytest.raises(ValueError, match="halo"):
                ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, *g.values(), 16, C1, C2)
        # window 7 needs 3 below / 3 above only: the same boxes pass
        ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, VOL, w0, wd, (12, 10, 27), (16, 8, 24), 7, C1, C2)
        with pytest.raises(ValueError):
            ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, *good.values(), 33, C1, C2)
        # an axis shorter than the ssim window must be in the window whole
        with pytest.raises(ValueError, match="whole"):
            ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, (37, 10, 70), (5, 2, 20), (32, 8, 50), (13, 2, 28), (16, 8, 24),
                               16, C1, C2)
        # what all three share: box outside the window or the volume, empty extents, a window that begins outside
        shared = [dict(b0=(4, 4, 27)), dict(bd=(33, 8, 24)), dict(bd=(16, 0, 24)), dict(wd=(32, 18, 0)),
                  dict(w0=(-1, 2, 20)), dict(vol=(37, 20, 60), b0=(13, 10, 40)), dict(vol=(37, 20, 0))]
        for case in shared:
            g = dict(good)
            g.update(case)
            with pytest.raises(ValueError):
                ctx.diff_histogram_u16(wins[0].ptr, wins[1].ptr, None, *g.values(), hist.ptr, zero_first=True)
            with pytest.raises(ValueError):
                ctx.mip3_u16(wins[0].ptr, wins[1].ptr, *g.values(), planes.ptr)
            with pytest.raises(ValueError):
                ctx.ssim3d_box_sum(wins[0].ptr, wins[1].ptr, *g.values(), 7, C1, C2)
        ctx.sync()
        hist.check_untouched("a rejected diff_histogram")          # not even zeroed: nothing was launched
        planes.check_untouched("a rejected mip3")
    finally:
        for v in wins + [hist, planes]:
            v.free()


# ---- evaluate.compare_stores --------------------------------------------------------------------------------------------
SHAPE = (45, 38, 52)
DELTA = 6
BRICKED, WHOLE = 500_000, 1 << 30          # budgets: 2 x 3 x 2 bricks with a mask (2 x 3 x 2 at 250 000 without), one brick


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """``ref`` (chunks 16, 16, 32), a bounded lossy and a lossless re-noised ``test`` (chunks 16, 32, 16) and a mask
    store, with their decoded arrays and the in-memory results, computed once."""
    base = tmp_path_factory.mktemp("compare-stores")
    vol, noisy = ref.synth_pair(SHAPE, seed=7)
    mask = (vol > np.percentile(vol, 85)).astype(U16)
    paths = {k: str(base / k) for k in ("ref", "lossy", "noisy", "mask")}
    ratios = {"ref": chunk_store.write_zarr(vol, paths["ref"], (1, 1, 16, 16, 32)),
              "lossy": chunk_store.write_zarr(vol, paths["lossy"], (1, 1, 16, 32, 16), codec=BoundedDctCodec(DELTA)),
              "noisy": chunk_store.write_zarr(noisy, paths["noisy"], (1, 1, 16, 32, 16))}
    chunk_store.write_zarr(mask, paths["mask"], (1, 1, 16, 16, 32))
    arrays = {k: chunk_store.read_zarr(p)[0, 0] for k, p in paths.items()}
    np.testing.assert_array_equal(arrays["ref"], vol)
    np.testing.assert_array_equal(arrays["noisy"], noisy)
    for v in arrays.values():
        v.setflags(write=False)
    return paths, arrays, ratios


def _same_but_ssim(got, want, what):
    """Everything that does not depend on the brick plan is equal."""
    for k in ("n", "mae", "mse", "bias", "lmax", "psnr", "data_range", "min", "max", "n_fg", "mae_fg", "mae_bg",
              "lmax_fg", "lmax_bg"):
        assert (k in got) == (k in want), (what, k)
        if k in want:
            assert got[k] == want[k], (what, k)
    for k in ("error_hist", "error_hist_fg", "error_hist_bg"):
        assert (k in got) == (k in want), (what, k)
        if k in want:
            assert got[k].dtype == np.uint64 and got[k].shape == (ref.DIFF_BINS,)
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    for name in ("ref", "test", "abs_diff"):
        for axis in range(3):
            assert got["mips"][name][axis].dtype == U16
            np.testing.assert_array_equal(got["mips"][name][axis], want["mips"][name][axis], err_msg=f"{what}: {name}")


def _check_against_numpy(res, a, b, mask, data_range, ssim_want):
    n = a.size
    d = b.astype(np.int64) - a.astype(np.int64)
    assert res["n"] == n
    np.testing.assert_array_equal(res["error_hist"], ref.diff_table(a, b, (0, 0, 0), a.shape))
    assert res["mae"] == img_util.compute_mae(a, b) == float(np.abs(d).sum() / n)
    assert res["lmax"] == img_util.compute_lmax(a, b) == int(np.abs(d).max())
    assert res["mse"] == int((d * d).sum()) / n and res["bias"] == int(d.sum()) / n
    assert res["min"] == {"ref": int(a.min()), "test": int(b.min())}
    assert res["max"] == {"ref": int(a.max()), "test": int(b.max())}
    want_mips = ref.whole_mips(a, b)
    for name in want_mips:
        for axis in range(3):
            np.testing.assert_array_equal(res["mips"][name][axis], want_mips[name][axis])
    if mask is not None:
        fg, bg = ref.diff_table(a, b, (0, 0, 0), a.shape, mask)
        np.testing.assert_array_equal(res["error_hist_fg"], fg)
        np.testing.assert_array_equal(res["error_hist_bg"], bg)
        m = mask != 0
        assert res["n_fg"] == int(m.sum())
        assert res["mae_fg"] == int(np.abs(d[m]).sum()) / int(m.sum())
        assert res["mae_bg"] == int(np.abs(d[~m]).sum()) / int((~m).sum())
        assert res["lmax_fg"] == int(np.abs(d[m]).max()) and res["lmax_bg"] == int(np.abs(d[~m]).max())
    assert res["data_range"] == float(data_range)
    print(f"ssim {res['ssim']!r} against ssim3D {ssim_want!r}")
    assert abs(res["ssim"] - ssim_want) <= 2 * n * 2.0 ** -53
    assert evaluate.abs_error_percentile(res["error_hist"], 99.9) == ref.abs_percentile(a, b, 99.9)


@pytest.mark.parametrize("test_store", ["lossy", "noisy"])
def test_compare_stores_two_passes(stores, test_store):
    """``data_range=None``: ssim3D's default range, which takes a second pass; with a mask store."""
    paths, arrays, ratios = stores
    a, b, mask = arrays["ref"], arrays[test_store], arrays["mask"]
    n = a.size
    plan = store_compare.plan_compare(SHAPE, (16, 16, 32), 16, BRICKED, True)
    assert all(len({br.origin[ax] for br in plan}) >= 2 for ax in range(3))
    stats = {}
    res = evaluate.compare_stores(paths["ref"], paths[test_store], mask=paths["mask"], budget_bytes=BRICKED, stats=stats)
    assert stats["bricks"] == len(plan) and stats["passes"] == 2
    assert stats["voxels_read"] == n + sum(br.window_voxels for br in plan) > 2 * n
    assert set(stats["seconds"]) == {"read", "histogram", "mips", "minmax", "ssim", "download"}
    assert stats["largest_alloc"] >= 3 * 2 * max(br.window_voxels for br in plan)
    lo, hi = (int(a.min()), int(b.min())), (int(a.max()), int(b.max()))
    data_range = max(float(hi[0]) - lo[0], float(hi[1]) - lo[1])
    _check_against_numpy(res, a, b, mask, data_range, float(img_util.ssim3D(a, b)))
    assert res["cratio_ref"] == ratios["ref"] and res["cratio_test"] == ratios[test_store]
    if test_store == "lossy":
        assert 0 < res["lmax"] <= DELTA          # the codec's guarantee, checked out of core
    # the arrays in memory, and the same call as one brick (StoredArrays instead of paths)
    in_memory = evaluate.compare_volumes(a, b, mask=mask)
    assert "cratio_ref" not in in_memory
    _same_but_ssim(res, in_memory, "compare_volumes")
    assert abs(res["ssim"] - in_memory["ssim"]) <= 2 * n * 2.0 ** -53
    one_stats = {}
    one = evaluate.compare_stores(chunk_store.open_zarr(paths["ref"]), chunk_store.open_zarr(paths[test_store]),
                                  mask=chunk_store.open_zarr(paths["mask"]), budget_bytes=WHOLE, stats=one_stats)
    assert one_stats["bricks"] == 1 and one_stats["voxels_read"] == 2 * n
    _same_but_ssim(res, one, "one brick")
    assert one["ssim"] == in_memory["ssim"] == float(img_util.ssim3D(a, b))     # one box: the whole-volume launch


@pytest.mark.parametrize("window_size", [16, 7])
def test_compare_stores_one_pass(stores, window_size):
    """A given ``data_range`` -- a number, and ``evaluate_blocks``' ``max(ref)`` -- takes one pass; no mask."""
    paths, arrays, _ = stores
    a, b = arrays["ref"], arrays["lossy"]
    n = a.size
    plan = store_compare.plan_compare(SHAPE, (16, 16, 32), window_size, BRICKED // 2, False)
    assert all(len({br.origin[ax] for br in plan}) >= 2 for ax in range(3))
    for data_range in (4000.0, np.max(a)):
        stats = {}
        res = evaluate.compare_stores(paths["ref"], paths["lossy"], data_range=data_range, window_size=window_size,
                                      budget_bytes=BRICKED // 2, stats=stats)
        assert stats["bricks"] == len(plan) and stats["passes"] == 1
        assert stats["voxels_read"] == sum(br.window_voxels for br in plan)
        assert "error_hist_fg" not in res and "mae_fg" not in res
        want = float(img_util.ssim3D(a, b, data_range=data_range, window_size=window_size))
        _check_against_numpy(res, a, b, None, data_range, want)
        assert res["psnr"] == 10.0 * math.log10(float(data_range) ** 2 / res["mse"])
        in_memory = evaluate.compare_volumes(a, b, data_range=data_range, window_size=window_size)
        _same_but_ssim(res, in_memory, "compare_volumes")
        assert in_memory["ssim"] == want


def test_compare_stores_of_a_store_with_itself(stores):
    paths, arrays, _ = stores
    res = evaluate.compare_stores(paths["ref"], paths["ref"], budget_bytes=BRICKED // 2)
    assert res["lmax"] == 0 and res["mae"] == 0.0 and res["psnr"] == float("inf") and res["bias"] == 0.0
    assert res["error_hist"][65535] == arrays["ref"].size == res["error_hist"].sum()
    assert res["ssim"] == pytest.approx(1.0, abs=1e-9) and not res["mips"]["abs_diff"][0].any()
    with pytest.raises(ValueError):
        evaluate.compare_stores(paths["ref"], paths["ref"], window_size=40)
