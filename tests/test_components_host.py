"""Connected-component filtering without a GPU: the pyref against scipy, the halo argument on the pyref
over real plans, the planner with ``min_voxels``, and the argument checks of every new keyword."""
import numpy as np
import pytest

import components_pyref as cref
import foreground_pyref as fref

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import store_compare, store_foreground
from aind_exaspim_image_compression.utils.store_predict import BRICK_BYTES, POOL_BYTES, window_slabs

U16 = np.uint16
CONNECTIVITIES = (6, 26)


# ---- the pyref against scipy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("density", (0.05, 0.2, 0.5))
def test_the_pyref_is_scipy_label(connectivity, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    seeds = np.random.default_rng(int(density * 100) + connectivity).random((22, 19, 27)) < density
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    want, n = ndimage.label(seeds, structure)
    lab = cref.labels(seeds, connectivity)
    assert cref.count_components(lab) == n
    got, got_n = cref.relabel(lab)
    assert got_n == n
    np.testing.assert_array_equal(got, want)                          # scipy's numbering, so the same partition
    flat = lab.reshape(-1)
    firsts = np.array([np.flatnonzero(want.reshape(-1) == i)[0] for i in range(1, n + 1)])
    np.testing.assert_array_equal(flat[firsts], firsts + 1)           # the canonical label is the first index + 1
    np.testing.assert_array_equal(cref.sizes(lab).reshape(-1)[firsts], np.bincount(want.reshape(-1))[1:])
    for m in (1, 2, 5):
        keep = np.concatenate([[False], np.bincount(want.reshape(-1))[1:] >= m])[want]
        np.testing.assert_array_equal(cref.kept(seeds, m, connectivity), keep)


def test_a_checkerboard_and_a_diagonal_are_singletons_under_6_and_one_under_26():
    shape = (5, 6, 7)
    z, y, x = np.indices(shape)
    for seeds in ((z + y + x) % 2 == 0, (z == y) & (y == x)):
        assert cref.count_components(cref.labels(seeds, 6)) == int(seeds.sum())
        assert cref.count_components(cref.labels(seeds, 26)) == 1


# ---- the halo argument: brick-wise equals whole -----------------------------------------------------------------------------
def _planted(shape, chunk, n, rng):
    """Sparse random seeds, and straight components of n - 1 and n voxels across the first brick face of every axis."""
    vol = (rng.random(shape) < 0.02).astype(U16) * 900
    at = {0: [(0, 2, 2), (0, 2, 6)], 1: [(16, 0, 10), (20, 0, 10)], 2: [(16, 16, 0), (20, 16, 0)]}
    lines = []
    for axis in range(3):
        for length, spot in zip((n - 1, n), at[axis]):
            start = chunk[axis] - (length + 1) // 2
            lines.append([tuple(start + t if a == axis else spot[a] for a in range(3)) for t in range(length)])
    for line in lines:                                     # nothing else touches a planted component
        for p in line:
            vol[tuple(slice(max(0, c - 1), c + 2) for c in p)] = 0
    for line in lines:
        for p in line:
            vol[p] = 900
    return vol


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("n", (1, 2, 3, 9))
def test_brick_wise_filtering_over_a_plan_is_the_whole_volume_filter(n, connectivity):
    shape, chunk, dilate = (23, 19, 31), (8, 8, 16), 1
    vol = _planted(shape, chunk, n, np.random.default_rng(10 * n + connectivity))
    seeds = vol >= 900
    lab = cref.labels(seeds, connectivity)
    comp_sizes = cref.sizes(lab).reshape(-1)
    comp_sizes = comp_sizes[comp_sizes > 0]
    assert (comp_sizes == n).any() and (n == 1 or (comp_sizes == n - 1).any())      # both sides of the rule are there
    whole = cref.filtered_mask(seeds, n, connectivity, dilate)
    bricks = store_foreground.plan_foreground(shape, chunk, dilate, 30_000, min_voxels=n)
    assert len(bricks) > 4
    got = np.zeros(shape, dtype=U16)
    sums = np.zeros(3, dtype=np.int64)
    fg = 0
    for b in bricks:
        lo, hi = cref.region(shape, b.origin, b.extent, dilate + 1)                 # the brick and its dilation halo
        dims = [h - l for l, h in zip(lo, hi)]
        rlo, rhi = cref.region(shape, lo, dims, n)
        for a in range(3):                                                         # the window holds what is labelled
            assert b.win_origin[a] <= rlo[a] and rhi[a] <= b.win_origin[a] + b.win_extent[a]
        res = cref.component_seeds(vol, 900, n, connectivity, lo, dims, b.origin, b.extent)
        sums += res["counts"]
        filtered = np.zeros(shape, dtype=U16)
        filtered[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = res["seeds_u16"]
        part, (_, f) = fref.box_mask(filtered, 1, dilate, b.origin, b.extent, 7)
        got[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] = part
        fg += f
    np.testing.assert_array_equal(got, whole.astype(U16) * 7)
    keep = cref.kept(seeds, n, connectivity)
    assert tuple(sums) == (int(seeds.sum()), int(keep.sum()), int((comp_sizes < n).sum()))
    assert fg == int(whole.sum())


# ---- the planner ------------------------------------------------------------------------------------------------------------
PLANS = [((40, 36, 70), (16, 16, 32)), ((40, 36, 70), (8, 16, 64)), ((45, 38, 52), (4, 16, 16)), ((7, 9, 5), (16, 16, 16)),
         ((33, 1, 129), (5, 1, 64))]


@pytest.mark.parametrize("min_voxels", (1, 2, 9, 64))
@pytest.mark.parametrize("dilate", (0, 2, 8))
@pytest.mark.parametrize("shape, chunk", PLANS)
def test_plan_foreground_with_min_voxels_by_brute_force(shape, chunk, dilate, min_voxels):
    halo = dilate + max(0, min_voxels - 1)
    seen_counts = set()
    for budget in (1, 400_000, 4_000_000, 4 << 30):
        bricks = store_foreground.plan_foreground(shape, chunk, dilate, budget, min_voxels=min_voxels)
        seen_counts.add(len(bricks))
        owner = np.zeros(shape, dtype=np.int32)
        for b in bricks:
            for o, e, c, n in zip(b.origin, b.extent, chunk, shape):
                assert o % c == 0 and (e % c == 0 or o + e == n) and e >= 1          # whole destination chunks
            owner[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] += 1
            for o, e, w0, wn, n in zip(b.origin, b.extent, b.win_origin, b.win_extent, shape):
                assert w0 == max(0, o - halo) and w0 + wn == min(n, o + e + halo)       # the halo, cut at the volume
            slabs, slab = window_slabs(b.win_extent[0], chunk[0])
            held = (slabs * slab, b.win_extent[1], b.win_extent[2])
            # what the loop holds at its peak: the window, the scratch of the labelled region, the filtered seeds
            s0, sd = _native.components_region(shape, b.origin, b.extent, dilate + 1)
            scratch = _native.components_scratch_bytes(_native.components_region(shape, s0, sd, min_voxels)[1])
            assert b.cost >= 2 * int(np.prod(held)) + scratch + 2 * int(np.prod(sd)) + 10 * int(np.prod(b.extent))
            assert scratch <= _native.components_scratch_bytes(held)
            single = all(e <= c for e, c in zip(b.extent, chunk))
            assert b.cost <= budget or single, (budget, b)
        assert (owner == 1).all()                                                      # a partition
    if int(np.prod([-(-s // c) for s, c in zip(shape, chunk)])) > 1:
        assert len(seen_counts) > 1                                                    # the budget matters


@pytest.mark.parametrize("dilate", (0, 1, 8))
@pytest.mark.parametrize("shape, chunk", PLANS)
def test_min_voxels_0_plans_are_the_old_plans(shape, chunk, dilate):
    for budget in (1, 40_000, 400_000, 4 << 30):
        old = store_compare.plan_bricks(shape, chunk, budget, 1, store_foreground.halo_window(dilate),
                                        BRICK_BYTES + POOL_BYTES)
        assert store_foreground.plan_foreground(shape, chunk, dilate, budget) == old
        assert store_foreground.plan_foreground(shape, chunk, dilate, budget, min_voxels=0) == old


def test_plan_foreground_rejects_a_bad_min_voxels():
    for bad in (-1, store_foreground.MAX_MIN_VOXELS + 1, 2.5, True):
        with pytest.raises(ValueError):
            store_foreground.plan_foreground((40, 36, 70), (16, 16, 32), 1, 1 << 20, min_voxels=bad)


def test_the_scratch_is_stated_without_a_gpu():
    assert store_foreground.MAX_MIN_VOXELS == 64 and _native.CC_TILE == (8, 8, 64)
    for name in ("exabm4d_components_scratch_bytes", "exabm4d_component_seeds_u16_dev", "exabm4d_label_components_dev"):
        assert name in _native.SIGNATURES
    for connectivity in CONNECTIVITIES:
        assert 3 * 4 * 60 <= _native.components_scratch_bytes((3, 4, 5), connectivity) <= 3 * 4 * 60 + 3 * 256
    for dims, connectivity in (((3, 4, 5), 18), ((0, 4, 5), 26), ((2048, 1024, 1024), 26)):
        with pytest.raises(ValueError):
            _native.components_scratch_bytes(dims, connectivity)
    assert _native.components_region((10, 10, 10), (2, 0, 5), (3, 4, 5), 3) == ((0, 0, 3), (7, 6, 7))
    assert metrics.label_components and metrics.remove_small_components


# ---- argument errors come before any context --------------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", refuse)
    monkeypatch.setattr(_native, "Context", refuse)


BAD = [dict(min_voxels=-1), dict(min_voxels=1.5), dict(min_voxels=True), dict(connectivity=18), dict(connectivity=8),
       dict(min_voxels=3, connectivity=0)]


@pytest.mark.parametrize("bad", BAD + [dict(min_voxels=65)])
def test_foreground_store_argument_errors_come_before_any_context(bad, tmp_path, no_context):
    with pytest.raises(ValueError):
        store_foreground.foreground_store(str(tmp_path / "no-such-store"), str(tmp_path / "dst"), device=0, **bad)
    assert not (tmp_path / "dst").exists()


@pytest.mark.parametrize("bad", BAD)
def test_in_memory_argument_errors_come_before_any_context(bad, no_context):
    vol = np.zeros((4, 5, 6), dtype=U16)
    with pytest.raises(ValueError):
        store_foreground.foreground_volume(vol, threshold=3.0, **bad)
    with pytest.raises(ValueError):
        metrics.make_foreground_mask(vol, **bad)
    with pytest.raises(ValueError):
        metrics.remove_small_components(vol != 0, **dict(dict(min_voxels=2), **bad))
    if "connectivity" in bad:
        with pytest.raises(ValueError):
            metrics.label_components(vol != 0, connectivity=bad["connectivity"])


def test_remove_small_components_argument_errors(no_context):
    for bad in (dict(mask=np.zeros((4, 5), dtype=bool), min_voxels=2), dict(mask=np.zeros((4, 0, 5), dtype=bool), min_voxels=2),
                dict(mask=np.zeros((4, 5, 6), dtype=bool), min_voxels=0)):
        with pytest.raises(ValueError):
            metrics.remove_small_components(**bad)
    with pytest.raises(ValueError):
        metrics.label_components(np.zeros(7, dtype=bool))
