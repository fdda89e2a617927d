"""The host side of ``downsample_label_store`` / ``pyramid_label_store`` / ``downsample_label_volume``,
no GPU: the brick plan by brute force, the argument checks that come before any context and write nothing, and where
the new names are."""
import numpy as np
import pytest

import label_pyramid_pyref as ref

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store, store_compare, store_label_pyramid, store_pyramid
from aind_exaspim_image_compression.utils.label_codec import LabelCodec
from aind_exaspim_image_compression.utils.store_predict import READER_SHARE, window_slabs

PLANS = [((45, 38, 67), (8, 8, 16)), ((40, 36, 70), (8, 16, 16)), ((7, 9, 5), (16, 16, 16)), ((33, 2, 129), (5, 1, 64))]


@pytest.mark.parametrize("typesize", [4, 8])
@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("factors", [(2, 2, 2), (1, 2, 2), (2, 1, 1), (1, 1, 2)])
@pytest.mark.parametrize("shape, chunk", PLANS)
def test_plan_label_downsample_by_brute_force(shape, chunk, factors, edge, typesize):
    want_level = ref.level_shape(shape, factors, edge)
    counts = set()
    for budget in (1, 30_000, 300_000, 4 << 30):
        level, bricks = store_label_pyramid.plan_label_downsample(shape, factors, edge, chunk, budget, typesize)
        assert level == want_level
        counts.add(len(bricks))
        owner = np.zeros(level, dtype=np.int32)
        for b in bricks:
            assert isinstance(b, store_compare.Brick)
            for o, e, c, n in zip(b.origin, b.extent, chunk, level):
                assert o % c == 0 and (e % c == 0 or o + e == n) and e >= 1              # whole destination chunks
            owner[tuple(slice(o, o + e) for o, e in zip(b.origin, b.extent))] += 1
            for o, e, w0, wn, f, n in zip(b.origin, b.extent, b.win_origin, b.win_extent, factors, shape):
                assert w0 == o * f and w0 + wn == min(n, (o + e) * f) and wn >= 1         # the source voxels under it
            slabs, slab = window_slabs(b.win_extent[0], chunk[0])
            held = slabs * slab * b.win_extent[1] * b.win_extent[2]
            assert b.cost == (typesize * held + budget // READER_SHARE +
                              (typesize + typesize + 1) * int(np.prod(b.extent)))
            single = all(e <= c for e, c in zip(b.extent, chunk))
            assert b.cost <= budget or single, (budget, b)
            if budget == 1:
                assert single
        assert (owner == 1).all()                                                          # a partition
        assert [b.origin for b in bricks] == sorted(b.origin for b in bricks)              # raster order
    assert len(bricks) == 1                                                                # 4 GiB hold these whole
    if int(np.prod([-(-s // c) for s, c in zip(want_level, chunk)])) > 1:
        assert len(counts) > 1                                                             # the budget matters


def test_the_cost_grows_with_the_typesize():
    args = ((40, 36, 70), (2, 2, 2), "crop", (8, 16, 16), 1)
    _, four = store_label_pyramid.plan_label_downsample(*args, 4)
    _, eight = store_label_pyramid.plan_label_downsample(*args, 8)
    # single-chunk bricks either way: the same boxes, each dearer at 8 bytes an element
    assert [b[:4] for b in four] == [b[:4] for b in eight] and len(four) == 3 * 2 * 3
    assert all(b8.cost > b4.cost for b4, b8 in zip(four, eight))
    # at one budget the wider elements give more bricks
    _, tight4 = store_label_pyramid.plan_label_downsample(*args[:4], 150_000, 4)
    _, tight8 = store_label_pyramid.plan_label_downsample(*args[:4], 150_000, 8)
    assert len(tight8) > len(tight4) > 1


def test_plan_label_downsample_rejects_bad_arguments():
    for bad in [dict(shape=(0, 4, 4)), dict(shape=(8, 8)), dict(chunks_zyx=(4, 4)), dict(chunks_zyx=(4, 0, 4)),
                dict(factors=(1, 1, 1)), dict(factors=(2, 4, 2)), dict(edge="reflect"), dict(budget_bytes=0),
                dict(typesize=2), dict(typesize=16), dict(shape=(1, 8, 8))]:              # crop: no level at all
        args = dict(shape=(40, 36, 70), factors=(2, 2, 2), edge="crop", chunks_zyx=(16, 16, 32), budget_bytes=1 << 20,
                    typesize=8)
        args.update(bad)
        with pytest.raises(ValueError):
            store_label_pyramid.plan_label_downsample(**args)


# ---- argument errors come before any context --------------------------------------------------------------------------------
@pytest.fixture
def no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", refuse)
    monkeypatch.setattr(_native, "Context", refuse)


BAD_RULE = [dict(factors=(1, 1, 1)), dict(factors=(2, 2)), dict(factors=(2, 3, 2)), dict(factors=(2, 2, 1.5)),
            dict(factors=None), dict(edge="pad"), dict(edge=None), dict(zeros="skip"), dict(zeros=1), dict(zeros=None)]
BAD_STORE = [dict(budget_bytes=0), dict(budget_bytes=None), dict(chunks=(16, 16, 32)), dict(chunks=(1, 2, 16, 16, 32)),
             dict(chunks=(1, 1, 0, 16, 32)), dict(chunks=7)]


@pytest.fixture
def label_src(tmp_path):
    src = str(tmp_path / "labels")
    chunk_store.create_zarr(src, (12, 10, 14), (1, 1, 8, 8, 8), codec=LabelCodec(8), device=0)
    return src


@pytest.mark.parametrize("bad", BAD_RULE + BAD_STORE, ids=repr)
def test_downsample_label_store_argument_errors_come_before_any_context(bad, tmp_path, no_context):
    args = dict(src=str(tmp_path / "no-such-store"), dst_path=str(tmp_path / "dst"), device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_label_pyramid.downsample_label_store(**args)
    assert not (tmp_path / "dst").exists()


def test_downsample_label_store_refuses_what_is_no_label_store(tmp_path, no_context, label_src):
    u16 = str(tmp_path / "u16")
    chunk_store.create_zarr(u16, (12, 10, 14), (1, 1, 8, 8, 8), device=0)
    dst = str(tmp_path / "dst")
    for src in (u16, chunk_store.open_zarr(u16, device=0), np.zeros((4, 4, 4), np.uint32), None, 7):
        with pytest.raises(ValueError, match="label"):
            chunk_store.downsample_label_store(src, dst, device=0)
        with pytest.raises(ValueError, match="label"):
            chunk_store.pyramid_label_store(src, dst, 2, device=0)
    with pytest.raises(ValueError, match="another device"):
        chunk_store.downsample_label_store(chunk_store.open_zarr(label_src, device=1), dst, device=0)
    # a source without a level: (1, 10, 14) under "crop"
    flat = str(tmp_path / "flat")
    chunk_store.create_zarr(flat, (1, 10, 14), (1, 1, 8, 8, 8), codec=LabelCodec(4), device=0)
    with pytest.raises(ValueError, match="no level"):
        chunk_store.downsample_label_store(flat, dst, device=0)
    assert not (tmp_path / "dst").exists()


@pytest.mark.parametrize("bad", BAD_RULE + [dict(vol=np.zeros((4, 4), np.uint32)), dict(vol=np.zeros((4, 4, 4), np.float32)),
                                            dict(vol=np.zeros((4, 4, 4), np.uint16)), dict(vol=np.zeros((4, 4, 4), np.int64)),
                                            dict(vol=np.zeros((4, 0, 4), np.uint64)),
                                            dict(vol=np.zeros((1, 4, 4), np.uint64), edge="crop")], ids=repr)
def test_downsample_label_volume_argument_errors_come_before_any_context(bad, no_context):
    args = dict(vol=np.zeros((4, 4, 4), np.uint64), factors=(2, 2, 2), edge="crop", zeros="count", device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_label_pyramid.downsample_label_volume(**args)


BAD_PYRAMID = [dict(n_levels=0), dict(n_levels=2.0), dict(n_levels=True), dict(factors=[(2, 2, 2)]),
               dict(factors=[(2, 2, 2), (2, 2, 2), (2, 2, 2)]), dict(factors=[(2, 2, 2), (1, 1, 1)]),
               dict(scale=[1, 1, 2, 2]), dict(translation=[0, 0, 0]), dict(translation="no"), dict(voxel_size=(1, 2)),
               dict(spatial_unit=3), dict(n_levels=6)]                                    # level 4 is (0, 0, 0)


@pytest.mark.parametrize("bad", BAD_RULE + BAD_STORE + BAD_PYRAMID, ids=repr)
def test_pyramid_label_store_argument_errors_come_before_any_context_and_write_nothing(bad, tmp_path, no_context,
                                                                                       label_src):
    args = dict(src=label_src, dst_path=str(tmp_path / "dst"), n_levels=3, device=0)
    args.update(bad)
    with pytest.raises(ValueError):
        store_label_pyramid.pyramid_label_store(**args)
    assert not (tmp_path / "dst").exists()


def test_the_new_names_are_where_their_siblings_are():
    for name in ("downsample_label_store", "downsample_label_volume", "pyramid_label_store", "plan_label_downsample"):
        assert getattr(chunk_store, name) is getattr(store_label_pyramid, name)
    assert "exabm4d_downsample_box_labels_dev" in _native.SIGNATURES
    assert _native.LABEL_ZEROS == {"count": 0, "ignore": 1}
    assert _native.DS_METHODS == {"mode": 0, "mean": 1, "max": 2} and _native.DS_EDGES == {"crop": 0, "partial": 1}
    assert store_label_pyramid.GROUP_TYPES == {"count": "mode", "ignore": "mode_nonzero"}
    assert store_pyramid.group_document([], "mode_nonzero")["attributes"]["ome"]["multiscales"][0]["type"] == "mode_nonzero"
