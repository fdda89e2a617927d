"""The host side of ``downsample_store`` / ``pyramid_store``, no GPU: level shapes, the brick plan by
brute force, the argument checks that come before any context, the group document against its formulas, and
``open_multiscale``."""
import json
import os

import numpy as np
import pytest

import pyramid_pyref as ref

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store, store_compare, store_pyramid
from aind_exaspim_image_compression.utils.store_predict import BRICK_BYTES, POOL_BYTES, READER_SHARE, window_slabs

ALL_FACTORS = [(2, 2, 2), (1, 2, 2), (2, 2, 1), (2, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 2)]


def test_level_shapes_for_both_edges():
    assert store_pyramid.level_shape((45, 38, 67), (2, 2, 2)) == (22, 19, 33)
    assert store_pyramid.level_shape((45, 38, 67), (2, 2, 2), "partial") == (23, 19, 34)
    assert store_pyramid.level_shape((45, 38, 67), (1, 2, 2), "crop") == (45, 19, 33)
    assert store_pyramid.level_shape((1, 2, 3), (2, 2, 2), "crop") == (0, 1, 1)
    assert store_pyramid.level_shape((1, 2, 3), (2, 2, 2), "partial") == (1, 1, 2)
    for shape in [(22, 19, 27), (9, 10, 131), (16, 16, 64), (1, 1, 1)]:
        for f in ALL_FACTORS:
            for edge in ref.EDGES:
                assert store_pyramid.level_shape(shape, f, edge) == ref.level_shape(shape, f, edge)
    for bad in [dict(factors=(1, 1, 1)), dict(factors=(2, 2)), dict(factors=(2, 3, 2)), dict(factors=(2, 2, 2.0)),
                dict(factors=(0, 2, 2)), dict(factors=7), dict(edge="pad"), dict(shape=(4, 4)), dict(shape=(0, 4, 4))]:
        args = dict(shape=(8, 8, 8), factors=(2, 2, 2), edge="crop")
        args.update(bad)
        with pytest.raises(ValueError):
            store_pyramid.level_shape(**args)


# ---- the planner by brute force -----------------------------------------------------------------------------------------
PLANS = [((45, 38, 67), (8, 8, 16)), ((40, 36, 70), (16, 16, 32)), ((7, 9, 5), (16, 16, 16)), ((33, 2, 129), (5, 1, 64)),
         ((64, 64, 64), (8, 16, 16))]


@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("factors", [(2, 2, 2), (1, 2, 2), (2, 2, 1), (2, 1, 1)])
@pytest.mark.parametrize("shape, chunk", PLANS)
def test_plan_downsample_by_brute_force(shape, chunk, factors, edge):
    seen_counts = set()
    want_level = ref.level_shape(shape, factors, edge)
    for budget in (1, 20_000, 200_000, 4 << 30):
        level, bricks = store_pyramid.plan_downsample(shape, factors, edge, chunk, budget)
        assert level == want_level
        seen_counts.add(len(bricks))
        owner = np.zeros(level, dtype=np.int32)
        for b in bricks:
            assert isinstance(b, store_compare.Brick)
            for o, e, c, n in zip(b.origin, b.extent, chunk, level):
                assert o % c == 0 and (e % c == 0 or o + e == n) and e >= 1              # whole destination chunks
            owner[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] += 1
            for o, e, w0, wn, f, n in zip(b.origin, b.extent, b.win_origin, b.win_extent, factors, shape):
                assert w0 == o * f and w0 + wn == min(n, (o + e) * f) and wn >= 1         # the source box, cut at the faces
            slabs, slab = window_slabs(b.win_extent[0], chunk[0])
            held = slabs * slab * b.win_extent[1] * b.win_extent[2]
            assert b.cost == (store_compare.WINDOW_BYTES * held + budget // READER_SHARE +
                              (BRICK_BYTES + POOL_BYTES) * int(np.prod(b.extent)))
            single = all(e <= c for e, c in zip(b.extent, chunk))
            assert b.cost <= budget or single, (budget, b)
        assert (owner == 1).all()                                                          # a partition
        assert [b.origin for b in bricks] == sorted(b.origin for b in bricks)              # raster order
    assert len(bricks) == 1                                                                # 4 GiB hold these whole
    if int(np.prod([-(-s // c) for s, c in zip(want_level, chunk)])) > 1:
        assert len(seen_counts) > 1                                                        # the budget matters


def test_plan_downsample_rejects_bad_arguments():
    for bad in [dict(shape=(0, 4, 4)), dict(shape=(8, 8)), dict(chunks_zyx=(4, 4)), dict(chunks_zyx=(4, 0, 4)),
                dict(factors=(1, 1, 1)), dict(factors=(2, 4, 2)), dict(edge="reflect"), dict(budget_bytes=0),
                dict(shape=(1, 8, 8))]:                                                   # crop: no level at all
        args = dict(shape=(40, 36, 70), factors=(2, 2, 2), edge="crop", chunks_zyx=(16, 16, 32), budget_bytes=1 << 20)
        args.update(bad)
        with pytest.raises(ValueError):
            store_pyramid.plan_downsample(**args)
    level, bricks = store_pyramid.plan_downsample((1, 8, 8), (2, 2, 2), "partial", (4, 4, 4), 1 << 20)
    assert level == (1, 4, 4) and len(bricks) == 1 and bricks[0].win_extent == (1, 8, 8)


def test_plan_bricks_with_one_window_function_is_what_it_was():
    """The per-axis extension leaves a single function alone: three copies of it plan the same bricks."""
    def window(b0, bd, dim):
        lo = max(0, b0 - 2)
        return lo, min(dim, b0 + bd + 2) - lo
    for budget in (1, 40_000, 4 << 30):
        one = store_compare.plan_bricks((40, 36, 70), (16, 16, 32), budget, 1, window, 10)
        three = store_compare.plan_bricks((40, 36, 70), (16, 16, 32), budget, 1, [window] * 3, 10)
        assert one == three and len(one) >= 1


# ---- argument errors come before any context --------------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", refuse)
    monkeypatch.setattr(_native, "Context", refuse)


BAD_RULE = [dict(factors=(1, 1, 1)), dict(factors=(2, 2)), dict(factors=(2, 3, 2)), dict(factors=(2, 2, 1.5)),
            dict(factors=None), dict(method="median"), dict(method=0), dict(edge="pad"), dict(edge=None)]
BAD_STORE = [dict(budget_bytes=0), dict(chunks=(16, 16, 32)), dict(chunks=(1, 2, 16, 16, 32)),
             dict(chunks=(1, 1, 0, 16, 32)), dict(chunks=7), dict(codec="zstd")]


@pytest.mark.parametrize("bad", BAD_RULE + BAD_STORE, ids=repr)
def test_downsample_store_argument_errors_come_before_any_context(bad, tmp_path, no_context):
    args = dict(src=str(tmp_path / "no-such-store"), dst_path=str(tmp_path / "dst"), device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_pyramid.downsample_store(**args)
    assert not (tmp_path / "dst").exists()


def test_downsample_store_refuses_a_source_without_a_level(tmp_path, no_context):
    src = str(tmp_path / "src")
    chunk_store.create_zarr(src, (1, 10, 14), (1, 1, 8, 8, 8), device=0)
    with pytest.raises(ValueError, match="no level"):
        chunk_store.downsample_store(src, str(tmp_path / "dst"), device=0)
    assert not (tmp_path / "dst").exists()


@pytest.mark.parametrize("bad", BAD_RULE + [dict(vol=np.zeros((4, 4), np.uint16)), dict(vol=np.zeros((4, 4, 4), np.float32)),
                                            dict(vol=np.zeros((4, 0, 4), np.uint16)),
                                            dict(vol=np.zeros((1, 4, 4), np.uint16), edge="crop")], ids=repr)
def test_downsample_volume_argument_errors_come_before_any_context(bad, no_context):
    args = dict(vol=np.zeros((4, 4, 4), np.uint16), factors=(2, 2, 2), method="mode", edge="crop", device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_pyramid.downsample_volume(**args)


BAD_PYRAMID = [dict(n_levels=0), dict(n_levels=2.0), dict(n_levels=True), dict(factors=[(2, 2, 2)]),
               dict(factors=[(2, 2, 2), (2, 2, 2), (2, 2, 2)]), dict(factors=[(2, 2, 2), (1, 1, 1)]),
               dict(scale=[1, 1, 2, 2]), dict(translation=[0, 0, 0]), dict(translation="no"), dict(voxel_size=(1, 2)),
               dict(spatial_unit=3), dict(n_levels=6)]                                    # level 4 is (0, 0, 0)


@pytest.mark.parametrize("bad", BAD_RULE + BAD_STORE + BAD_PYRAMID, ids=repr)
def test_pyramid_store_argument_errors_come_before_any_context_and_write_nothing(bad, tmp_path, no_context):
    src = str(tmp_path / "src")
    chunk_store.create_zarr(src, (12, 10, 14), (1, 1, 8, 8, 8), device=0)
    args = dict(src=src, dst_path=str(tmp_path / "dst"), n_levels=3, device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_pyramid.pyramid_store(**args)
    assert not (tmp_path / "dst").exists()


# ---- the group document -------------------------------------------------------------------------------------------------------
def _check_document(doc, steps, method, base_scale, base_translation, unit):
    assert doc["zarr_format"] == 3 and doc["node_type"] == "group"
    (ms,) = doc["attributes"]["ome"]["multiscales"]
    assert ms["type"] == method
    assert ms["axes"] == [{"name": "t", "type": "time", "unit": "millisecond"}, {"name": "c", "type": "channel"},
                          {"name": "z", "type": "space", "unit": unit}, {"name": "y", "type": "space", "unit": unit},
                          {"name": "x", "type": "space", "unit": unit}]
    assert [d["path"] for d in ms["datasets"]] == [str(k) for k in range(len(steps) + 1)]
    cumulative = np.ones(5)
    for k, d in enumerate(ms["datasets"]):
        if k:
            cumulative = cumulative * np.array((1, 1) + tuple(steps[k - 1]), dtype=float)
        scale = np.asarray(base_scale, dtype=float) * cumulative
        translation = np.asarray(base_translation, dtype=float) + (scale - np.asarray(base_scale, dtype=float)) / 2
        s, t = d["coordinateTransformations"]
        assert s == {"type": "scale", "scale": scale.tolist()}
        assert t == {"type": "translation", "translation": translation.tolist()}
    json.dumps(doc)


def test_the_group_document_follows_the_formulas():
    steps = [(2, 2, 2)] * 3
    tr = store_pyramid.level_transforms(steps)
    assert tr[0] == ([1.0, 1.0, 1000.0, 748.0, 748.0], [0.0] * 5)
    assert tr[1] == ([1.0, 1.0, 2000.0, 1496.0, 1496.0], [0.0, 0.0, 500.0, 374.0, 374.0])
    assert tr[3] == ([1.0, 1.0, 8000.0, 5984.0, 5984.0], [0.0, 0.0, 3500.0, 2618.0, 2618.0])
    _check_document(store_pyramid.group_document(tr, "mode"), steps, "mode", [1, 1, 1000, 748, 748], [0] * 5, "nanometer")
    # one triple per step, a given scale and translation, another unit
    steps = [(1, 2, 2), (2, 2, 2)]
    scale, translation = [1, 1, 2.0, 0.5, 0.5], [0, 0, 10.0, -3.0, 7.5]
    tr = store_pyramid.level_transforms(steps, scale=scale, translation=translation)
    assert tr[1] == ([1.0, 1.0, 2.0, 1.0, 1.0], [0.0, 0.0, 10.0, -2.75, 7.75])
    assert tr[2] == ([1.0, 1.0, 4.0, 2.0, 2.0], [0.0, 0.0, 11.0, -2.25, 8.25])
    _check_document(store_pyramid.group_document(tr, "max", "micrometer"), steps, "max", scale, translation, "micrometer")
    assert store_pyramid._level_factors(3, steps) == steps and store_pyramid._level_factors(3, (2, 2, 1)) == [(2, 2, 1)] * 2
    assert store_pyramid._level_factors(1, (2, 2, 2)) == []


# ---- open_multiscale ------------------------------------------------------------------------------------------------------------
def test_open_multiscale_round_trip(tmp_path):
    """A group whose level arrays are made as empty stores: ``open_multiscale`` reads documents only."""
    root = tmp_path / "group"
    steps = [(1, 2, 2), (2, 2, 2)]
    shapes = [(12, 10, 14), (12, 5, 7), (6, 2, 3)]
    os.makedirs(root)
    for k, shape in enumerate(shapes):
        chunk_store.create_zarr(str(root / str(k)), shape, (1, 1, 8, 8, 8), device=0)
    with pytest.raises(FileNotFoundError):
        chunk_store.open_multiscale(str(root), device=0)                  # a group without its document is incomplete
    tr = store_pyramid.level_transforms(steps, voxel_size=(3, 4, 5))
    with open(root / "zarr.json", "w") as f:
        json.dump(store_pyramid.group_document(tr, "mean"), f)
    levels, transforms = chunk_store.open_multiscale(str(root), device=0)
    assert [tuple(a.shape) for a in levels] == [(1, 1) + s for s in shapes]
    assert transforms == tr and transforms[2] == ([1.0, 1.0, 10.0, 16.0, 12.0], [0.0, 0.0, 2.5, 6.0, 4.5])
    with pytest.raises(ValueError):
        chunk_store.open_multiscale(str(root / "0"), device=0)            # an array, not a group


def test_the_new_names_are_where_their_siblings_are():
    assert chunk_store.downsample_store is store_pyramid.downsample_store
    assert chunk_store.pyramid_store is store_pyramid.pyramid_store
    assert chunk_store.open_multiscale is store_pyramid.open_multiscale
    assert "exabm4d_downsample_box_u16_dev" in _native.SIGNATURES
    assert _native.DS_METHODS == {"mode": 0, "mean": 1, "max": 2} and _native.DS_EDGES == {"crop": 0, "partial": 1}
