"""Pyramid levels of label stores on the MI355X: ``exabm4d_downsample_box_labels_dev`` in guarded,
poisoned buffers against the numpy rule (``label_pyramid_pyref``) -- both dtypes, both ``zeros``, every factor triple,
both edges, windows and outputs of every alignment, padding past the faces that would win every vote --, the argument
checks, ``downsample_label_volume``, ``downsample_label_store`` against ``write_zarr`` chunk file for chunk file,
``pyramid_label_store`` level by level with its group document, and the level of a ``components_store``."""
import itertools
import json
import os

import numpy as np
import pytest

import label_pyramid_pyref as ref
from util import GuardedView

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import chunk_store, store_label_pyramid, store_pyramid
from aind_exaspim_image_compression.utils.label_codec import LabelCodec
from aind_exaspim_image_compression.utils.store_labels import LabelArray

pytestmark = pytest.mark.gpu
FACTORS = [f for f in itertools.product((1, 2), repeat=3) if max(f) == 2]
DTYPES = (np.uint32, np.uint64)
BIG_IDS = {np.uint32: [1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1],
           np.uint64: [1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1]}
# three values each; the likelier value is sometimes the smaller and sometimes the larger one, so that the smaller
# loses on frequency in some windows and wins ties in others
ALPHABETS = {
    np.uint32: {"0 and ids >= 2^31": ([0, 2 ** 31, 2 ** 31 + 1], [0.4, 0.25, 0.35]),
                "1, 2^31, 2^32 - 1": ([1, 2 ** 31, 2 ** 32 - 1], [0.3, 0.4, 0.3]),
                "small": ([0, 3, 9], [0.5, 0.2, 0.3])},
    np.uint64: {"only the high word differs": ([1, 2 ** 32 + 1, 2 ** 63 + 1], [0.3, 0.4, 0.3]),
                "only the low word differs": ([2 ** 32, 2 ** 32 + 1, 2 ** 32 + 2], [0.3, 0.3, 0.4]),
                "0, 2^32 - 1, 2^63": ([0, 2 ** 32 - 1, 2 ** 63], [0.45, 0.25, 0.3]),
                "2^32, 2^64 - 1, 2^63": ([2 ** 32, 2 ** 64 - 1, 2 ** 63], [0.3, 0.4, 0.3])},
}
_CACHE = {}


def _volumes(shape, dtype):
    """Named volumes of ``shape``, read-only and made once."""
    key = (shape, dtype)
    if key not in _CACHE:
        rng = np.random.default_rng(sum(shape) + np.dtype(dtype).itemsize)
        vols = {}
        for name, (values, p) in ALPHABETS[dtype].items():
            vols[name] = rng.choice(np.array(values, dtype=dtype), size=shape, p=p)
        for v in vols.values():
            assert v.dtype == dtype
            v.setflags(write=False)
        _CACHE[key] = vols
    return _CACHE[key]


def _level(shape, dtype, name, factors, edge, zeros):
    """The pyref level of a named volume, computed once and shared."""
    key = (shape, dtype, name, factors, edge, zeros)
    if key not in _CACHE:
        level = ref.downsample(_volumes(shape, dtype)[name], factors, edge, zeros)
        level.setflags(write=False)
        _CACHE[key] = level
    return _CACHE[key]


def _window(vol, origin, dims, fill):
    """The window ``origin + [0, dims)`` of ``vol``; what lies past the volume's faces holds ``fill``."""
    out = np.full(dims, fill, dtype=vol.dtype)
    inside = tuple(slice(0, min(d, n - o)) for o, d, n in zip(origin, dims, vol.shape))
    out[inside] = vol[tuple(slice(o, o + s.stop) for o, s in zip(origin, inside))]
    return out


def _run(ctx, vol, want_level, w0, wd, b0, bd, factors, edge, zeros, k=0, out_k=0, fill=0, what=""):
    """One call in guarded, poisoned buffers, checked against the box of ``want_level``."""
    want = ref.box(want_level, b0, bd)
    assert want.shape == tuple(bd)
    win = GuardedView(ctx, vol.dtype, int(np.prod(wd)), k=k, data=_window(vol, w0, wd, fill))
    out = GuardedView(ctx, vol.dtype, int(np.prod(bd)), k=out_k)
    try:
        ctx.downsample_box_labels(win.ptr, vol.dtype, vol.shape, w0, wd, b0, bd, factors, edge, zeros, out=out.ptr)
        ctx.sync()
        out.check_output(want, f"{what}: out")
        win.check_untouched(f"{what}: window")
    finally:
        win.free()
        out.free()


def _rules():
    return itertools.product(FACTORS, ref.EDGES, ref.ZEROS)


# ---- the entry against the pyref ------------------------------------------------------------------------------------------
SHAPE = (13, 11, 37)
# (window origin, window dims -- SOURCE --, box origin, box dims -- LEVEL; None: the whole level --, pointer offsets)
CASES = {
    "the whole level, pitch 37": ((0, 0, 0), SHAPE, None, None, 0, 0),
    "the whole level, pointers + 1 element": ((0, 0, 0), SHAPE, None, None, 1, 1),
    "the whole level, window + 2 elements, output + 1": ((0, 0, 0), SHAPE, None, None, 2, 1),
    "the whole level past the faces, pitch 40 (vector loads)": ((0, 0, 0), (14, 12, 40), None, None, 0, 0),
    "the whole level past the faces, pitch 40, window + 1, output + 2": ((0, 0, 0), (14, 12, 40), None, None, 1, 2),
    # the box's source is [2, 8) x [2, 8) x [6, 16) at factors of 2 and [1, 4) x [1, 4) x [3, 8) at factors of 1
    "an inner box at odd origins, pitch 15, 5 voxels a row (element loads and stores)":
        ((1, 1, 3), (8, 8, 15), (1, 1, 3), (3, 3, 5), 0, 0),
    # [2, 8) x [2, 8) x [8, 24) or [1, 4) x [1, 4) x [4, 12): phase 0 in a window that begins at x = 4
    "an inner box, pitch 20, aligned pointers, 8 voxels a row (vector loads and stores)":
        ((1, 1, 4), (8, 8, 20), (1, 1, 4), (3, 3, 8), 0, 0),
    "an inner box, pitch 20, window + 1 element, output + 1": ((1, 1, 4), (8, 8, 20), (1, 1, 4), (3, 3, 8), 1, 1),
    "an inner box, pitch 20, window + 2 elements, output + 2": ((1, 1, 4), (8, 8, 20), (1, 1, 4), (3, 3, 8), 2, 2),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", list(CASES))
def test_boxes_of_every_alignment(ctx, case, dtype):
    w0, wd, b0, bd, k, out_k = CASES[case]
    for factors, edge, zeros in _rules():
        level_shape = ref.level_shape(SHAPE, factors, edge)
        box0, boxd = (b0, bd) if b0 is not None else ((0, 0, 0), level_shape)
        for name, vol in _volumes(SHAPE, dtype).items():
            # a window past the faces is padded with 1: non-zero and no larger than any id, so it would win where read
            _run(ctx, vol, _level(SHAPE, dtype, name, factors, edge, zeros), w0, wd, box0, boxd, factors, edge, zeros,
                 k=k, out_k=out_k, fill=1, what=f"{case}, {name}, {factors} {edge} {zeros}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(6, 10, 600), (4, 140, 18)], ids=str)
def test_more_pieces_than_a_wave_and_several_rows_a_wave(ctx, shape, dtype):
    """(6, 10, 600): level rows of 300 (600) voxels, more pieces than a wave has lanes; (4, 140, 18): a level of
    2 x 70 x 9, rows of a few pieces that share a wave."""
    for factors, edge, zeros in _rules():
        level_shape = ref.level_shape(shape, factors, edge)
        for name, vol in list(_volumes(shape, dtype).items())[:2]:
            _run(ctx, vol, _level(shape, dtype, name, factors, edge, zeros), (0, 0, 0), shape, (0, 0, 0), level_shape,
                 factors, edge, zeros, what=f"{shape} {name}, {factors} {edge} {zeros}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_last_voxels_of_a_partial_level_beside_poisoned_padding(ctx, dtype):
    """(7, 9, 11) in a window of (8, 10, 12): the last windows hold 1, 2 or 4 voxels beside a reader's padding.  Every
    id of the volume is >= 2 and the padding holds 1: non-zero, smaller than every id (it would win every tie) and as
    frequent as the voxels present or more so."""
    shape, wd = (7, 9, 11), (8, 10, 12)
    rng = np.random.default_rng(5)
    vol = rng.choice(np.array([2] + BIG_IDS[dtype][1:], dtype=dtype), size=shape)
    for factors, zeros in itertools.product(FACTORS, ref.ZEROS):
        want = ref.downsample(vol, factors, "partial", zeros)
        assert want.min() >= 2
        last = tuple(n - 1 for n in want.shape)
        for b0, bd in ((last, (1, 1, 1)), ((0, 0, 0), want.shape)):
            _run(ctx, vol, want, (0, 0, 0), wd, b0, bd, factors, "partial", zeros, fill=1,
                 what=f"box {b0} + {bd}, {factors} {zeros}")


# ---- argument errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_bad_arguments_are_refused_and_nothing_is_written(ctx, dtype):
    shape, ts = (22, 19, 27), np.dtype(dtype).itemsize
    b0, bd = (2, 2, 2), (5, 4, 6)                          # source voxels (4, 4, 4) + (10, 8, 12)
    w0, wd = (3, 3, 3), (12, 10, 14)
    win = GuardedView(ctx, dtype, int(np.prod(wd)) + 8, data=np.zeros(int(np.prod(wd)) + 8, dtype=dtype))
    out = GuardedView(ctx, dtype, int(np.prod(bd)) + 1)
    fn = _native.lib().exabm4d_downsample_box_labels_dev
    invalid = -1                                           # EXABM4D_ERR_INVALID

    def raw(typesize=ts, shape=shape, w0=w0, wd=wd, b0=b0, bd=bd, factors=(2, 2, 2), edge=0, zeros=0, pw=None, po=None):
        tri = ctx._box_geometry(shape, w0, wd, b0, bd)
        fac = (_native.ctypes.c_int32 * 3)(*factors)
        return fn(ctx.handle, win.ptr if pw is None else pw, typesize, *tri, fac, edge, zeros,
                  out.ptr if po is None else po)

    try:
        assert raw() == 0                                  # the geometry itself is accepted
        ctx.sync()
        out.buf.upload(out.host)                           # poison it again
        bad = [dict(typesize=2), dict(typesize=0), dict(typesize=16), dict(zeros=7), dict(zeros=-1), dict(edge=2),
               dict(b0=(9, 2, 2)),                         # a box outside the "crop" level of 11 x 9 x 13
               dict(b0=(2, 2, 8)), dict(bd=(5, 8, 6)),
               dict(w0=(5, 3, 3)),                         # the window begins after the box's source
               dict(wd=(12, 10, 12)),                      # the window ends before the box's source does
               dict(pw=win.ptr + ts // 2), dict(po=out.ptr + ts // 2), dict(pw=win.ptr + 1),
               dict(factors=(1, 1, 1)), dict(factors=(2, 3, 2)), dict(shape=((1 << 20) + 1, 19, 27)),
               dict(w0=(-1, 3, 3)), dict(bd=(0, 4, 6))]
        for kw in bad:
            assert raw(**kw) == invalid, kw
        for kw in (dict(zeros="skip"), dict(edge="pad"), dict(factors=(2, 2, 4))):
            args = dict(factors=(2, 2, 2), edge="crop", zeros="count")
            args.update(kw)
            with pytest.raises(ValueError):
                ctx.downsample_box_labels(win.ptr, dtype, shape, w0, wd, b0, bd, out=out.ptr, **args)
        with pytest.raises(ValueError):
            ctx.downsample_box_labels(win.ptr, np.uint16, shape, w0, wd, b0, bd, (2, 2, 2), out=out.ptr)
        with pytest.raises(ValueError):
            ctx.downsample_box_labels(win.ptr, np.int64, shape, w0, wd, b0, bd, (2, 2, 2), out=out.ptr)
        ctx.sync()
        out.check_untouched("after the refused calls")
        win.check_untouched("after the refused calls")
    finally:
        win.free()
        out.free()


# ---- downsample_label_volume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape, rules", [((21, 18, 45), [(2, 2, 2), (1, 2, 2), (2, 1, 2)]), ((1, 16, 64), [(1, 2, 2)]),
                                          ((8, 8, 8), [(2, 2, 2), (2, 2, 1)])], ids=str)
def test_downsample_label_volume_is_the_pyref(shape, rules, dtype):
    for name, vol in _volumes(shape, dtype).items():
        for factors, edge, zeros in itertools.product(rules, ref.EDGES, ref.ZEROS):
            got = store_label_pyramid.downsample_label_volume(vol, factors, edge, zeros)
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, _level(shape, dtype, name, factors, edge, zeros),
                                          err_msg=f"{name} {factors} {edge} {zeros}")


# ---- downsample_label_store against write_zarr, chunk file for chunk file ---------------------------------------------------
STORE_SHAPE, SRC_CHUNKS, DST_CHUNKS = (40, 36, 70), (1, 1, 16, 16, 32), (1, 1, 8, 16, 16)
BUDGETS = {"one chunk per brick": 1, "a few bricks of several chunks": 400_000, "one brick": 4 << 30}
STORE_RULES = list(itertools.product(((2, 2, 2), (1, 2, 2)), ref.EDGES, ref.ZEROS))


def _segmentation(dtype):
    """Blocky regions, lines one voxel thin, a corner of small-alphabet noise, and the large ids."""
    rng = np.random.default_rng(23)
    ids = BIG_IDS[dtype]
    vol = np.zeros(STORE_SHAPE, dtype=dtype)
    vol[4:22, 3:20, 5:40] = ids[1]
    vol[10:30, 12:33, 30:66] = ids[2]
    vol[25:40, 0:9, 0:21] = ids[3]
    vol[0:7, 20:36, 50:70] = ids[-1]
    vol[13, 7, :] = ids[-2]                                # lines one voxel thin, through regions and background
    vol[:, 29, 11] = 77
    vol[33, :, 45] = ids[0]
    vol[31:40, 27:36, 55:70] = rng.choice(np.array([0, ids[1], ids[-1]], dtype=dtype), size=(9, 9, 15))
    vol.setflags(write=False)
    return vol


def _files(path):
    out = {}
    for dirpath, _, names in os.walk(path):
        for name in names:
            full = os.path.join(dirpath, name)
            with open(full, "rb") as f:
                out[os.path.relpath(full, path)] = f.read()
    return out


def _assert_same_store(got, want, what):
    a, b = _files(got), _files(want)
    assert sorted(a) == sorted(b), f"{what}: the directory listings differ"
    assert len(a) > 1 and "zarr.json" in a
    for name in a:
        assert a[name] == b[name], f"{what}: {name} differs"


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """Per dtype the source store, its array, and ``write_zarr`` of the pyref level of every rule, made once."""
    root = tmp_path_factory.mktemp("label_pyramid")
    out = {}
    for dtype in DTYPES:
        name = np.dtype(dtype).name
        vol = _segmentation(dtype)
        codec = LabelCodec(np.dtype(dtype).itemsize)
        src = str(root / f"src_{name}")
        chunk_store.write_zarr(vol, src, SRC_CHUNKS, codec=codec)
        want = {}
        for i, (factors, edge, zeros) in enumerate(STORE_RULES):
            level = ref.downsample(vol, factors, edge, zeros)
            want[factors, edge, zeros] = (str(root / f"want_{name}_{i}"), level.shape)
            chunk_store.write_zarr(level, want[factors, edge, zeros][0], DST_CHUNKS, codec=codec)
        out[dtype] = {"src": src, "vol": vol, "want": want}
    return out


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_downsample_label_store_is_write_zarr_of_the_level(stored, tmp_path, dtype, budget):
    ts = np.dtype(dtype).itemsize
    for i, (factors, edge, zeros) in enumerate(STORE_RULES):
        want_path, want_shape = stored[dtype]["want"][factors, edge, zeros]
        _, bricks = store_label_pyramid.plan_label_downsample(STORE_SHAPE, factors, edge, DST_CHUNKS[2:], BUDGETS[budget],
                                                              ts)
        n_chunks = int(np.prod([-(-s // c) for s, c in zip(want_shape, DST_CHUNKS[2:])]))
        assert len(bricks) == {"one chunk per brick": n_chunks, "one brick": 1}.get(budget, len(bricks))
        assert budget != "a few bricks of several chunks" or 1 < len(bricks) < n_chunks
        dst, stats = str(tmp_path / f"dst_{i}"), {}
        res = chunk_store.downsample_label_store(stored[dtype]["src"], dst, factors, edge, zeros, chunks=DST_CHUNKS,
                                                 budget_bytes=BUDGETS[budget], stats=stats)
        _assert_same_store(dst, want_path, f"{factors} {edge} {zeros}")
        assert res["shape"] == want_shape and res["n"] == int(np.prod(want_shape)) and res["cratio"] > 1
        assert stats["bricks"] == len(bricks)
        assert stats["voxels_read"] == sum(b.window_voxels for b in bricks)
        assert set(stats["seconds"]) == {"read", "reduce", "encode", "files_write"}
        # at least a window with its dense brick
        assert stats["largest_alloc"] >= max(ts * (b.window_voxels + int(np.prod(b.extent))) for b in bricks)
        assert isinstance(chunk_store.open_zarr(dst), LabelArray)


def test_downsample_label_store_takes_an_open_array_and_the_sources_chunks(stored, tmp_path):
    arr = chunk_store.open_zarr(stored[np.uint64]["src"])
    dst = str(tmp_path / "dst")
    res = chunk_store.downsample_label_store(arr, dst, zeros="ignore", attributes={"note": "level 1"})
    got = chunk_store.open_zarr(dst)
    assert tuple(got.chunks) == (1, 1, 16, 16, 32) and got.dtype == np.uint64 and res["shape"] == (20, 18, 35)
    np.testing.assert_array_equal(got[0, 0], ref.downsample(stored[np.uint64]["vol"], (2, 2, 2), "crop", "ignore"))
    assert got.meta["attributes"]["note"] == "level 1"


# ---- the multiscale group -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, zeros", [(np.uint64, "ignore"), (np.uint32, "count")], ids=str)
def test_pyramid_label_store_level_by_level(stored, tmp_path, dtype, zeros):
    steps = [(2, 2, 2), (1, 2, 2)]
    vol, src = stored[dtype]["vol"], stored[dtype]["src"]
    codec = LabelCodec(np.dtype(dtype).itemsize)
    dst, stats = str(tmp_path / "pyramid"), {}
    res = chunk_store.pyramid_label_store(src, dst, 3, steps, "partial", zeros, chunks=DST_CHUNKS, voxel_size=(3, 4, 5),
                                          budget_bytes=400_000, stats=stats)
    want0 = str(tmp_path / "want0")
    chunk_store.write_zarr(vol, want0, DST_CHUNKS, codec=codec)
    _assert_same_store(os.path.join(dst, "0"), want0, "level 0")
    levels, transforms = chunk_store.open_multiscale(dst)
    assert len(levels) == 3 and all(isinstance(a, LabelArray) and a.dtype == dtype for a in levels)
    before = vol
    for k, arr in enumerate(levels):
        if k:
            before = ref.downsample(before, steps[k - 1], "partial", zeros)
        np.testing.assert_array_equal(arr[0, 0], before, err_msg=f"level {k}")
        assert tuple(arr.shape) == (1, 1) + before.shape == (1, 1) + res["shapes"][k]
    assert res["shapes"] == [(40, 36, 70), (20, 18, 35), (20, 9, 18)]
    assert transforms == res["transforms"] == store_pyramid.level_transforms(steps, voxel_size=(3, 4, 5))
    with open(os.path.join(dst, "zarr.json")) as f:
        doc = json.load(f)
    kind = {"count": "mode", "ignore": "mode_nonzero"}[zeros]
    assert doc == store_pyramid.group_document(transforms, kind)
    assert len(res["cratios"]) == 3 and len(stats["levels"]) == 3 and stats["levels"][0]["bricks"] > 1


def test_a_pyramid_too_deep_and_a_pyramid_that_fails(stored, tmp_path, monkeypatch):
    src = stored[np.uint32]["src"]
    # (40, 36, 70) -> ... -> (1, 1, 2) -> (0, 0, 1) under "crop": level 6 has an empty axis
    deep = str(tmp_path / "deep")
    with pytest.raises(ValueError, match="level 6"):
        chunk_store.pyramid_label_store(src, deep, 7, chunks=DST_CHUNKS)
    assert not os.path.exists(deep)
    # an old group document goes first: a run that fails at a later level leaves an incomplete group
    dst = str(tmp_path / "pyramid")
    chunk_store.pyramid_label_store(src, dst, 2, chunks=DST_CHUNKS)
    assert os.path.exists(os.path.join(dst, "zarr.json"))
    plan, calls = store_label_pyramid._plan, []

    def failing(who, *args):
        calls.append(who)
        if len(calls) == 3:                                # level 0, level 1, then level 2
            raise RuntimeError("no plan for this level")
        return plan(who, *args)

    monkeypatch.setattr(store_label_pyramid, "_plan", failing)
    with pytest.raises(RuntimeError, match="no plan"):
        chunk_store.pyramid_label_store(src, dst, 3, chunks=DST_CHUNKS)
    assert not os.path.exists(os.path.join(dst, "zarr.json")) and os.path.exists(os.path.join(dst, "1", "zarr.json"))


# ---- the end of the chain ---------------------------------------------------------------------------------------------------------
def test_the_level_of_a_components_store_holds_ids_of_its_size_table(tmp_path):
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 60, (24, 20, 40)).astype(np.uint16)
    vol[2:9, 3:12, 4:30] = 900                             # a block
    vol[15, 10, :] = 700                                   # a line one voxel thin
    vol[12:24, 17, 33] = 800
    vol[20:23, 2:5, 2:5] = 500
    src, labels, dst = str(tmp_path / "src"), str(tmp_path / "labels"), str(tmp_path / "level")
    chunk_store.write_zarr(vol, src, (1, 1, 8, 16, 16))
    res = metrics.components_store(src, labels, threshold=100, connectivity=26, budget_bytes=1)
    assert res["n_kept_components"] == 4
    out = chunk_store.downsample_label_store(labels, dst, zeros="ignore", budget_bytes=1)
    level = chunk_store.open_zarr(dst)[0, 0]
    assert out["shape"] == (12, 10, 20) == level.shape
    np.testing.assert_array_equal(level, ref.downsample(chunk_store.read_zarr(labels)[0, 0], (2, 2, 2), "crop", "ignore"))
    found = np.unique(level[level != 0])
    assert found.size == 4 and np.isin(found, res["labels"]).all()      # the thin lines are still there
