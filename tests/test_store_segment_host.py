"""Out-of-core component labelling without a GPU: the numpy restatement of the whole scheme against
whole-volume labelling, ``merge_records`` on the cases that strain it, ``plan_segment`` and the argument errors."""
import numpy as np
import pytest

import segment_pyref
from aind_exaspim_image_compression.utils import store_segment
from aind_exaspim_image_compression.utils.store_segment import final_labels, merge_records, plan_segment

CASES = [((20, 24, 70), (8, 8, 32)), ((9, 17, 33), (4, 8, 16)), ((16, 16, 16), (16, 16, 16)), ((4, 5, 6), (1, 1, 1))]


def _mask(shape, density, seed=0):
    return np.random.default_rng(seed).random(shape) < density


# ---- the whole scheme, restated in numpy ----------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("density", [0.05, 0.3, 0.9])
@pytest.mark.parametrize("shape,brick", CASES)
def test_bricks_and_merge_equal_whole_volume_labelling(shape, brick, density, connectivity):
    seeds = _mask(shape, density, seed=shape[2] + int(100 * density))
    want, want_labels, want_sizes = segment_pyref.whole_volume(seeds, connectivity)
    got, labels, sizes = segment_pyref.components(seeds, brick, connectivity)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(labels, want_labels)
    np.testing.assert_array_equal(sizes, want_sizes)                  # exact sizes: no halo voxel is counted twice
    np.testing.assert_array_equal(sizes, np.bincount(want.reshape(-1).astype(np.int64))[want_labels.astype(np.int64)])


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_vectorised_merge_is_the_union_find(connectivity):
    seeds = _mask((9, 17, 33), 0.3, seed=5)
    a = segment_pyref.components(seeds, (4, 8, 16), connectivity)
    b = segment_pyref.components(seeds, (4, 8, 16), connectivity, merge=segment_pyref.merge_by_loops)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("min_voxels,relabel", [(2, False), (65, False), (0, True), (3, True)])
def test_min_voxels_and_relabel_through_the_bricks(min_voxels, relabel):
    seeds = _mask((9, 17, 33), 0.3, seed=7)
    want = segment_pyref.whole_volume(seeds, 6, min_voxels, relabel)
    got = segment_pyref.components(seeds, (4, 8, 16), 6, min_voxels, relabel)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)


def test_the_pyref_window_labeller_is_the_repositorys_canonical_labelling():
    import components_pyref
    seeds = _mask((6, 7, 9), 0.4, seed=1)
    for connectivity in (6, 26):
        np.testing.assert_array_equal(segment_pyref.first_voxel_labels(seeds, connectivity),
                                      components_pyref.labels(seeds, connectivity))


# ---- merge_records --------------------------------------------------------------------------------------------------
def _chain(n):
    """Labels 10, 20, .. 10 n, each owning one voxel; label i is joined to label i - 1 through voxel 1000 + i, and
    the records come in descending order: the minimum has to travel the whole chain."""
    labels = np.arange(n, 0, -1, dtype=np.uint64) * 10
    size = np.stack([labels, np.ones(n, np.uint64)], axis=1)
    vox = 1000 + np.arange(n - 1, 0, -1, dtype=np.uint64)
    halo = np.stack([vox, labels[:-1]], axis=1)                       # the upper label sees the voxel as halo
    face = np.stack([vox, labels[1:]], axis=1)                        # the lower one owns it
    return halo, face, size


def test_a_long_chain_collapses_to_its_minimum():
    halo, face, size = _chain(3000)
    keys, vals, table = merge_records(halo, face, size)
    np.testing.assert_array_equal(keys, np.arange(1, 3001, dtype=np.uint64) * 10)
    assert np.all(vals == 10)
    np.testing.assert_array_equal(table, [[10, 3000]])
    for got, want in zip((keys, vals, table), segment_pyref.merge_by_loops(halo, face, size)):
        np.testing.assert_array_equal(got, want)


def test_duplicate_halo_and_face_records_change_nothing():
    halo, face, size = _chain(50)
    twice = merge_records(np.concatenate([halo, halo[::3]]), np.concatenate([face[::2], face]), size)
    for got, want in zip(twice, merge_records(halo, face, size)):
        np.testing.assert_array_equal(got, want)


def test_one_label_reported_by_two_bricks_adds_its_sizes():
    size = np.array([[7, 3], [9, 1], [7, 4]], dtype=np.uint64)
    keys, vals, table = merge_records(np.zeros((0, 2)), np.zeros((0, 2)), size)
    np.testing.assert_array_equal(keys, [7, 9])
    np.testing.assert_array_equal(vals, [7, 9])
    np.testing.assert_array_equal(table, [[7, 7], [9, 1]])


def test_empty_input():
    empty = np.zeros((0, 2), dtype=np.uint64)
    keys, vals, table = merge_records(empty, empty, empty)
    assert keys.size == 0 and vals.size == 0 and table.shape == (0, 2)
    assert keys.dtype == np.uint64 and table.dtype == np.uint64
    assert final_labels(table, 5, True).size == 0


def test_a_halo_voxel_without_a_face_record_is_a_plan_bug():
    halo, face, size = _chain(5)
    with pytest.raises(RuntimeError, match="no face record"):
        merge_records(halo, face[1:], size)
    with pytest.raises(RuntimeError, match="no face record"):
        merge_records(halo, np.zeros((0, 2), np.uint64), size)
    with pytest.raises(ValueError):
        merge_records(np.zeros(3, np.uint64), face, size)


def test_labels_past_2_pow_32_survive():
    big = np.uint64(2 ** 40)
    halo = np.array([[5, big + np.uint64(8)]], dtype=np.uint64)
    face = np.array([[5, big + np.uint64(2)]], dtype=np.uint64)
    size = np.array([[big + np.uint64(8), 2], [big + np.uint64(2), 1]], dtype=np.uint64)
    keys, vals, table = merge_records(halo, face, size)
    np.testing.assert_array_equal(vals, [big + np.uint64(2)] * 2)
    np.testing.assert_array_equal(table, [[big + np.uint64(2), 3]])


def test_min_voxels_and_relabel_on_the_table():
    table = np.array([[3, 5], [10, 1], [11, 2], [40, 9]], dtype=np.uint64)
    np.testing.assert_array_equal(final_labels(table), [3, 10, 11, 40])
    np.testing.assert_array_equal(final_labels(table, 1), [3, 10, 11, 40])
    np.testing.assert_array_equal(final_labels(table, 2), [3, 0, 11, 40])
    np.testing.assert_array_equal(final_labels(table, 1000), [0, 0, 0, 0])
    np.testing.assert_array_equal(final_labels(table, 0, True), [1, 2, 3, 4])
    np.testing.assert_array_equal(final_labels(table, 5, True), [1, 0, 0, 2])
    assert final_labels(table, 5, True).dtype == np.uint64


# ---- plan_segment ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,chunk,budget", [((20, 24, 70), (8, 8, 32), 1), ((20, 24, 70), (8, 8, 32), 4 << 30),
                                                ((100, 90, 130), (16, 16, 32), 6 << 20), ((5, 5, 5), (8, 8, 8), 1 << 20),
                                                ((64, 64, 64), (16, 16, 16), 24 << 20)])
def test_plan_segment(shape, chunk, budget):
    bricks = plan_segment(shape, chunk, budget, 4)
    seen = np.zeros(shape, dtype=np.int32)
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    for b in bricks:
        sl = tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))
        seen[sl] += 1
        for a in range(3):
            assert b.origin[a] % chunk[a] == 0                                 # whole destination chunks
            assert b.extent[a] % chunk[a] == 0 or b.origin[a] + b.extent[a] == shape[a]
            assert b.win_origin[a] == b.origin[a]                              # nothing on the low side
            assert b.win_extent[a] == min(shape[a], b.origin[a] + b.extent[a] + 1) - b.origin[a]
        single = all(e <= c for e, c in zip(b.extent, chunk))
        assert b.cost <= budget or single
    assert np.all(seen == 1)                                                   # the bricks partition the volume
    if budget == 1:
        assert len(bricks) == grid[0] * grid[1] * grid[2]
    if budget == 4 << 30:
        assert len(bricks) == 1
    if shape == (100, 90, 130):
        assert 1 < len(bricks) < grid[0] * grid[1] * grid[2]                   # the budget shapes the bricks


def test_no_budget_buys_a_window_of_2_pow_31_voxels():
    bricks = plan_segment((2048, 2048, 2048), (128, 128, 128), 1 << 44, 8)
    assert len(bricks) > 1
    assert max(b.window_voxels for b in bricks) < 2 ** 31
    assert sum(int(np.prod(b.extent)) for b in bricks) == 2048 ** 3


def test_plan_segment_arguments():
    with pytest.raises(ValueError):
        plan_segment((4, 4), (2, 2, 2), 100, 4)
    with pytest.raises(ValueError):
        plan_segment((4, 4, 4), (2, 2, 0), 100, 4)
    with pytest.raises(ValueError):
        plan_segment((4, 4, 4), (2, 2, 2), 0, 4)
    with pytest.raises(ValueError):
        plan_segment((4, 4, 4), (2, 2, 2), 100, 2)


def test_record_capacities_are_the_geometric_worst_case():
    from aind_exaspim_image_compression import _native
    seeds = np.ones((9, 10, 11), dtype=bool)
    for origin, extent, window in segment_pyref.bricks_of(seeds.shape, (4, 5, 6)):
        halo, face, _, _ = segment_pyref.collect(seeds, origin, extent, window, 26)
        assert _native.segment_record_capacities(window, origin, extent) == (len(halo), len(face))


# ---- argument errors, without a device ------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [{"connectivity": 18}, {"min_voxels": -1}, {"min_voxels": 1.5}, {"min_voxels": True},
                                    {"dtype": np.int32}, {"dtype": np.uint16}, {"dtype": "labels"},
                                    {"budget_bytes": 0}, {"chunks": (8, 8, 8)}, {"chunks": (1, 1, 8, 0, 8)},
                                    {"chunks": 7}, {"measure": object()}, {"threshold": float("nan")},
                                    {"k": -1.0, "threshold": None}, {"k": float("inf"), "threshold": None}])
def test_components_store_argument_errors_need_no_device(tmp_path, kwargs, monkeypatch):
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.machine_learning import metrics

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before a context exists")

    monkeypatch.setattr(_native, "context", no_device)
    kwargs.setdefault("threshold", 10)
    with pytest.raises(ValueError):
        metrics.components_store(str(tmp_path / "missing.zarr"), str(tmp_path / "dst.zarr"), **kwargs)
    assert not (tmp_path / "dst.zarr").exists()


def test_components_volume_argument_errors_need_no_device(monkeypatch):
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.machine_learning import metrics
    monkeypatch.setattr(_native, "context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("no device")))
    mask = np.ones((4, 4, 4), dtype=bool)
    for kwargs in ({"connectivity": 8}, {"min_voxels": -2}, {"dtype": np.int64}, {"brick": (2, 2)}, {"brick": (2, 0, 2)}):
        with pytest.raises(ValueError):
            metrics.components_volume(mask, **kwargs)
    with pytest.raises(ValueError):
        metrics.components_volume(np.ones((4, 4), dtype=bool))
    with pytest.raises(ValueError):
        metrics.components_volume(np.ones((4, 4, 4), dtype=np.float32))


def test_the_label_type_follows_the_volume():
    assert store_segment._label_dtype("t", None, 2 ** 32 - 1, False) == 4
    assert store_segment._label_dtype("t", None, 2 ** 32, False) == 8
    assert store_segment._label_dtype("t", np.uint64, 10, False) == 8
    assert store_segment._label_dtype("t", np.uint32, 2 ** 32, True) == 4          # (checked again after the merge)
    with pytest.raises(ValueError, match="do not fit uint32"):
        store_segment._label_dtype("t", np.uint32, 2 ** 32, False)
