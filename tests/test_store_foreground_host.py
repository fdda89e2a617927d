"""The host side of ``foreground_store`` / ``recode_store``, no GPU: the threshold that follows from a
table of the counts against numpy's own median arithmetic, the brick plan by brute force, the brick-wise pyref against
the whole-volume dilation, and the argument checks that come before any context."""
import numpy as np
import pytest

import foreground_pyref as ref
import mask_pyref

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store, store_foreground, store_measure, store_recode
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
from aind_exaspim_image_compression.utils.store_predict import window_slabs

U16 = np.uint16


def _measure_of(vol):
    counts = np.bincount(vol.reshape(-1), minlength=store_measure.COUNT_BINS)
    return store_measure.StoreMeasure(vol.shape, counts, np.zeros((store_measure.LEVELS, store_measure.WIDE_BINS), np.uint64),
                                      np.zeros(store_measure.LEVELS, np.uint64))


def _populations():
    rng = np.random.default_rng(11)
    bimodal = np.where(rng.random((9, 8, 10)) < 0.6, rng.integers(90, 130, (9, 8, 10)), rng.integers(3000, 60000, (9, 8, 10)))
    even = np.array([3, 3, 3, 4, 9, 9, 50, 700], dtype=U16).reshape(2, 2, 2)            # middle values 4 and 9: median 6.5
    return {
        "odd n": rng.poisson(200, (5, 3, 7)).astype(U16),
        "even n, half-integer median": even,
        "constant": np.full((4, 5, 6), 321, dtype=U16),
        "values 0..2": rng.integers(0, 3, (6, 7, 5)).astype(U16),
        "values 65530..65535": rng.integers(65530, 65536, (6, 5, 7)).astype(U16),
        "bimodal": bimodal.astype(U16),
    }


POPULATIONS = _populations()


@pytest.mark.parametrize("name", list(POPULATIONS))
def test_threshold_and_cut_follow_from_the_counts(name):
    vol = POPULATIONS[name]
    m = _measure_of(vol)
    raw = vol.astype(np.float32)
    ks = (0, 0.5, 6) + ((1e9,) if name == "values 65530..65535" else ())
    for k in ks:
        want = mask_pyref.fg_threshold(vol, k)
        got = m.foreground_threshold(k)
        assert type(got) is np.float32 and got == want, (name, k, got, want)
        assert ref.threshold_from_counts(m.counts, k) == want
        cut = m.foreground_cut(k)
        assert 0 <= cut <= 65536 and cut == ref.cut_from_counts(m.counts, k)
        np.testing.assert_array_equal(vol.astype(np.int64) >= cut, raw > want, err_msg=f"{name}, k={k}")
    if name == "even n, half-integer median":
        assert float(np.median(raw)) == 6.5
    if name == "constant":
        assert m.foreground_cut(6) == 322 and m.foreground_cut(0) == 322       # MAD 0: the threshold is med + k 1.48e-6
    if name == "values 65530..65535":
        assert m.foreground_threshold(6) > 65535 and m.foreground_cut(6) == 65536 and m.foreground_cut(1e9) == 65536
        assert not (raw > mask_pyref.fg_threshold(vol, 6)).any()


@pytest.mark.parametrize("k", [-1.0, -1e-9, float("nan"), float("inf"), float("-inf")])
def test_a_bad_k_is_refused(k):
    m = _measure_of(POPULATIONS["odd n"])
    with pytest.raises(ValueError):
        m.foreground_threshold(k)
    with pytest.raises(ValueError):
        m.foreground_cut(k)


# ---- the planner by brute force -----------------------------------------------------------------------------------------
PLANS = [((40, 36, 70), (16, 16, 32)), ((40, 36, 70), (8, 16, 64)), ((45, 38, 52), (4, 16, 16)), ((7, 9, 5), (16, 16, 16)),
         ((33, 1, 129), (5, 1, 64))]


@pytest.mark.parametrize("dilate", (0, 1, 2, 8))
@pytest.mark.parametrize("shape, chunk", PLANS)
def test_plan_foreground_by_brute_force(shape, chunk, dilate):
    seen_counts = set()
    for budget in (1, 40_000, 400_000, 4 << 30):
        bricks = store_foreground.plan_foreground(shape, chunk, dilate, budget)
        seen_counts.add(len(bricks))
        owner = np.zeros(shape, dtype=np.int32)
        for i, b in enumerate(bricks):
            for o, e, c, n in zip(b.origin, b.extent, chunk, shape):
                assert o % c == 0 and (e % c == 0 or o + e == n) and e >= 1          # whole destination chunks
            owner[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] += 1
            for o, e, w0, wn, n in zip(b.origin, b.extent, b.win_origin, b.win_extent, shape):
                assert w0 == max(0, o - dilate) and w0 + wn == min(n, o + e + dilate)   # the ball, cut at the volume
            slabs, slab = window_slabs(b.win_extent[0], chunk[0])
            held = slabs * slab * b.win_extent[1] * b.win_extent[2]
            assert b.cost >= 2 * held + 10 * int(np.prod(b.extent))
            single = all(e <= c for e, c in zip(b.extent, chunk))
            assert b.cost <= budget or single, (budget, b)
        assert (owner == 1).all()                                                      # a partition
    if int(np.prod([-(-s // c) for s, c in zip(shape, chunk)])) > 1:
        assert len(seen_counts) > 1                                                    # the budget matters


def test_plan_foreground_rejects_bad_arguments():
    for bad in [dict(shape=(0, 4, 4)), dict(chunks_zyx=(4, 4)), dict(dilate=-1), dict(dilate=9), dict(budget_bytes=0)]:
        args = dict(shape=(40, 36, 70), chunks_zyx=(16, 16, 32), dilate=1, budget_bytes=1 << 20)
        args.update(bad)
        with pytest.raises(ValueError):
            store_foreground.plan_foreground(**args)


# ---- the brick-wise pyref is the whole-volume dilation --------------------------------------------------------------------
@pytest.mark.parametrize("radius", (0, 1, 2, 3, 8))
def test_box_masks_over_a_plan_are_the_whole_volume_mask(radius):
    rng = np.random.default_rng(radius)
    shape, chunk = (22, 19, 27), (8, 8, 16)
    vol = (rng.random(shape) < 0.01).astype(U16) * 900
    for z in (0, shape[0] - 1):                            # and the corners
        for y in (0, shape[1] - 1):
            for x in (0, shape[2] - 1):
                vol[z, y, x] = 900
    whole = mask_pyref.dilate(vol >= 900, radius)
    np.testing.assert_array_equal(ref.ball_dilate(vol >= 900, radius), whole)
    got = np.zeros(shape, dtype=U16)
    seeds = fg = 0
    bricks = store_foreground.plan_foreground(shape, chunk, radius, 30_000)
    assert len(bricks) > 4
    for b in bricks:
        part, (s, f) = ref.box_mask(vol, 900, radius, b.origin, b.extent, 7)
        got[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] = part
        seeds, fg = seeds + s, fg + f
    np.testing.assert_array_equal(got, whole.astype(U16) * 7)
    assert seeds == int((vol >= 900).sum()) and fg == int(whole.sum())


@pytest.mark.parametrize("radius", (0, 1, 2, 3, 8))
def test_the_ball_is_scipy_binary_dilation(radius):
    ndimage = pytest.importorskip("scipy.ndimage")
    seeds = np.random.default_rng(radius).random((22, 19, 27)) < 0.01
    seeds[0, 0, 0] = seeds[-1, -1, -1] = True
    want = ndimage.binary_dilation(seeds, iterations=radius) if radius else seeds
    np.testing.assert_array_equal(ref.ball_dilate(seeds, radius), want)
    np.testing.assert_array_equal(ref.box_mask(seeds.astype(U16), 1, radius, (3, 0, 5), (19, 19, 20))[0], want[3:, :, 5:25])


# ---- argument errors come before any context --------------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", refuse)
    monkeypatch.setattr(_native, "Context", refuse)


@pytest.mark.parametrize("bad", [dict(dilate=-1), dict(dilate=9), dict(value=0), dict(value=65536), dict(budget_bytes=0),
                                 dict(chunks=(16, 16, 32)), dict(chunks=(1, 2, 16, 16, 32)), dict(chunks=(1, 1, 0, 16, 32)),
                                 dict(chunks=7), dict(k=-1.0), dict(k=float("nan")), dict(threshold=float("inf")),
                                 dict(measure="not a measurement")])
def test_foreground_store_argument_errors_come_before_any_context(bad, tmp_path, no_context):
    args = dict(src=str(tmp_path / "no-such-store"), dst_path=str(tmp_path / "dst"), device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_foreground.foreground_store(**args)
    assert not (tmp_path / "dst").exists()


def test_recode_store_argument_errors_come_before_any_context(tmp_path, no_context):
    src, other = str(tmp_path / "src"), str(tmp_path / "other")
    chunk_store.create_zarr(src, (12, 10, 14), (1, 1, 8, 8, 8), device=0)
    chunk_store.create_zarr(other, (12, 10, 15), (1, 1, 8, 8, 8), device=0)
    dst = str(tmp_path / "dst")
    with pytest.raises(ValueError, match="takes a mask"):                      # what write_zarr raises
        store_recode.recode_store(src, dst, codec=ExacCodec(2), mask=src, device=0)
    with pytest.raises(ValueError, match="takes a mask"):
        chunk_store.recode_store(src, dst, mask=src, device=0)
    with pytest.raises(ValueError, match="one shape"):
        store_recode.recode_store(src, dst, codec=BlockBoundedCodec(16, 0), mask=other, device=0)
    for bad in (dict(budget_bytes=0), dict(chunks=(8, 8, 8))):
        with pytest.raises(ValueError):
            store_recode.recode_store(src, dst, device=0, **bad)
    assert not (tmp_path / "dst").exists()


def test_the_new_names_are_where_their_siblings_are():
    from aind_exaspim_image_compression.machine_learning import metrics
    assert metrics.foreground_store is store_foreground.foreground_store
    assert metrics.foreground_volume is store_foreground.foreground_volume
    assert chunk_store.recode_store is store_recode.recode_store
    assert _native.FG_MAX_RADIUS == 8 and store_foreground.MAX_DILATE == 8
    assert "exabm4d_foreground_box_u16_dev" in _native.SIGNATURES and "exabm4d_nonzero_u8_dev" in _native.SIGNATURES
