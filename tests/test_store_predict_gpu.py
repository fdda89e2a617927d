"""BM4DNet inference store to store on the MI355X: the two brick kernels
(``exabm4d_tile_gather_u16_dev``, ``exabm4d_tile_stitch_u16_dev``) bit for bit against tests/stitch_pyref.py, in
guarded buffers, and ``inference.predict_store`` against ``predict`` + ``write_zarr``: byte equality for a model whose
output rows do not depend on the batch, and for the real U-Net within what ``predict`` itself moves when only its
batch size changes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import region_write_pyref as wref
import stitch_pyref
from test_oracle_golden import TRANSFORM_CFGS
from util import GuardedView, synth_volume

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.inference import predict, predict_store
from aind_exaspim_image_compression.machine_learning import transforms as T
from aind_exaspim_image_compression.machine_learning.unet3d import UNet
from aind_exaspim_image_compression.utils import chunk_store, store_predict
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec

pytestmark = pytest.mark.gpu
F32 = np.float32

# the four transform configurations of the stream-kernel tests: asinh, anscombe, linear, offset
CFGS = ["asinh_s32_o35", "anscombe_g8_rn5_o100", "linear_35_1000_8", "offset37_asinh_s32"]
SHAPE = (45, 38, 52)
GEOMETRY = (16, 6, 2)                              # patch, overlap, trim: stride 10, core 12, 4 x 4 x 5 patches


def _counts(shape, seed):
    """uint16 counts over the whole range, the ends included."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, shape).astype(np.uint16)
    v.reshape(-1)[:4] = [0, 65535, 1, 32768]
    return v


def _grid_starts(first, count, stride):
    return [tuple((first[a] + i[a]) * stride for a in range(3)) for i in np.ndindex(*count)]


# ---- kernel a: exabm4d_tile_gather_u16_dev ----------------------------------------------------------------------
def _gather(ctx, name, vol, origin, dims, first, count, batches, geometry=GEOMETRY):
    patch, overlap, _ = geometry
    cfg = TRANSFORM_CFGS[name]
    tf = T.build_transform(cfg).native_struct()
    grid = _native.patch_grid(first, count, patch - overlap, patch)
    starts = _grid_starts(first, count, patch - overlap)
    win = np.ascontiguousarray(vol[tuple(slice(o, o + d) for o, d in zip(origin, dims))])
    assert win.shape == tuple(dims)
    d_win = ctx.to_device(win)
    try:
        for k0, nb in batches:
            want = stitch_pyref.gather_patches(vol, cfg, patch, starts[k0:k0 + nb])
            out = GuardedView(ctx, F32, nb * patch ** 3)
            try:
                ctx.tile_gather_u16(tf, d_win, origin, dims, vol.shape, grid, k0, nb, out.ptr)
                ctx.sync()
                out.check_output(want, f"tile_gather_u16 {name} k0={k0} nb={nb}")
            finally:
                out.free()
    finally:
        d_win.free()


@pytest.mark.parametrize("name", CFGS)
def test_tile_gather_u16_window(ctx, name):
    """The window (30, 38, 26) at (10, 0, 20): patches 1..2 x 0..3 x 2..3, the last y patch padded; batches that
    start and end in the middle of a row of the grid."""
    _gather(ctx, name, _counts(SHAPE, 1), (10, 0, 20), (30, 38, 26), (1, 0, 2), (2, 4, 2),
            [(0, 16), (1, 5), (3, 7), (15, 1)])


def test_tile_gather_u16_whole_volume(ctx):
    """The volume as its own window and the whole grid: the last z and y patches are padded."""
    _gather(ctx, "asinh_s32_o35", _counts(SHAPE, 2), (0, 0, 0), SHAPE, (0, 0, 0), (4, 4, 5), [(7, 13), (67, 13)])


def test_tile_gather_u16_rejects_a_wrong_plan(ctx):
    vol = _counts(SHAPE, 3)
    tf = T.build_transform(TRANSFORM_CFGS["asinh_s32_o35"]).native_struct()
    grid = _native.patch_grid((1, 0, 2), (2, 4, 2), 10, 16)
    d_win = ctx.to_device(np.ascontiguousarray(vol[10:40, :, 20:46]))
    out = GuardedView(ctx, F32, 7 * 16 ** 3)
    try:
        bad = [dict(dims=(25, 38, 26)),                                # the window ends before its patches do
               dict(dims=(30, 37, 26)),                                # ... before the volume's face in y
               dict(origin=(11, 0, 20)),                               # ... begins behind the first patch
               dict(k0=10, nb=7), dict(k0=-1, nb=2), dict(k0=16, nb=1)]    # the batch runs past the grid
        for case in bad:
            a = dict(origin=(10, 0, 20), dims=(30, 38, 26), k0=0, nb=7)
            a.update(case)
            with pytest.raises(ValueError):
                ctx.tile_gather_u16(tf, d_win, a["origin"], a["dims"], SHAPE, grid, a["k0"], a["nb"], out.ptr)
            ctx.sync()
            out.check_untouched(str(case))
    finally:
        out.free()
        d_win.free()


# ---- kernel b: exabm4d_tile_stitch_u16_dev ----------------------------------------------------------------------
def _predictions(n, patch, seed):
    """fp32 outputs of a network: mostly in and around [0, 1], negative values, -0.0, and values far beyond the
    transforms' range on both sides, which saturate the quantiser."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.3, 1.3, (n, patch, patch, patch)).astype(F32)
    r = rng.random(p.shape)
    p[r < 0.05] = F32(-0.0)
    p[(r >= 0.05) & (r < 0.08)] = F32(1e4)             # 1e4 * (mx - mn) of the linear transform is past 65535 too
    p[(r >= 0.08) & (r < 0.11)] = F32(-1e4)
    return p


_STITCHED = {}


def _stitched(name, shape, geometry):
    """(predictions, the whole volume's counts per stitch_pyref) of a case, computed once and read-only."""
    key = (name, shape, geometry)
    if key not in _STITCHED:
        patch, overlap, trim = geometry
        starts = stitch_pyref.patch_starts(shape, patch, overlap)
        preds = _predictions(len(starts), patch, 11)
        want = stitch_pyref.stitch(preds, starts, shape, trim, TRANSFORM_CFGS[name])
        preds.setflags(write=False)
        want.setflags(write=False)
        _STITCHED[key] = (preds, want)
    return _STITCHED[key]


def _stitch(ctx, name, shape, geometry, origin, extent, sub_grid=False):
    patch, overlap, trim = geometry
    preds, want = _stitched(name, shape, geometry)
    full = tuple(store_predict.axis_patches(n, patch, overlap) for n in shape)
    first, count = (0, 0, 0), full
    if sub_grid:                                       # only the patches the box needs, as predict_store passes them
        fc = [store_predict.patch_range(o, o + e, n, patch, overlap, trim) for o, e, n in zip(origin, extent, shape)]
        first, count = tuple(f for f, _ in fc), tuple(c for _, c in fc)
        idx = [np.ravel_multi_index(tuple(first[a] + i[a] for a in range(3)), full) for i in np.ndindex(*count)]
        preds = preds[idx] if idx else preds[:0]
    tf = T.build_transform(TRANSFORM_CFGS[name]).native_struct()
    grid = _native.patch_grid(first, count, patch - overlap, patch)
    d_preds = ctx.to_device(preds if len(preds) else np.zeros(1, F32))
    out = GuardedView(ctx, np.uint16, int(np.prod(extent)))
    try:
        ctx.tile_stitch_u16(tf, d_preds if len(preds) else None, len(preds), grid, trim, origin, extent, shape,
                            out.ptr)
        ctx.sync()
        out.check_output(want[tuple(slice(o, o + e) for o, e in zip(origin, extent))],
                         f"tile_stitch_u16 {name} {origin} {extent}")
    finally:
        out.free()
        d_preds.free()
    return want


@pytest.mark.parametrize("name", CFGS)
def test_tile_stitch_u16_whole_volume(ctx, name):
    """... and the existing pair tile_accumulate + tile_finalize on the same predictions gives the same counts."""
    want = _stitch(ctx, name, SHAPE, GEOMETRY, (0, 0, 0), SHAPE)
    assert want[:2].min() == want[:2].max() == want[44].min() == want[44].max()       # no core there: inverse(0)
    assert want.max() == 65535 and len(np.unique(want)) > 100      # the quantiser saturates; the rest is spread out
    preds, _ = _stitched(name, SHAPE, GEOMETRY)
    starts = stitch_pyref.patch_starts(SHAPE, GEOMETRY[0], GEOMETRY[1])
    n = int(np.prod(SHAPE))
    bufs = [ctx.to_device(preds), ctx.alloc(4 * n).zero(), ctx.alloc(4 * n).zero(), ctx.alloc(2 * n)]
    try:
        ctx.tile_accumulate(bufs[0], starts, GEOMETRY[0], GEOMETRY[2], bufs[1], bufs[2], SHAPE)
        ctx.tile_finalize(T.build_transform(TRANSFORM_CFGS[name]).native_struct(), bufs[1], bufs[2], bufs[3], n)
        ctx.sync()
        np.testing.assert_array_equal(bufs[3].download(SHAPE, np.uint16), want)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("sub_grid", [False, True])
@pytest.mark.parametrize("origin,extent", [
    ((7, 5, 9), (20, 17, 25)),                         # an interior box whose faces cut through core overlaps
    ((44, 0, 0), (1, 38, 52)),                         # the slab no core reaches
    ((13, 12, 23), (1, 1, 1)),                         # one voxel, in the overlap of two cores on every axis
])
def test_tile_stitch_u16_boxes(ctx, origin, extent, sub_grid):
    _stitch(ctx, "offset37_asinh_s32", SHAPE, GEOMETRY, origin, extent, sub_grid)


@pytest.mark.parametrize("sub_grid", [False, True])
def test_tile_stitch_u16_three_patches_deep(ctx, sub_grid):
    """Geometry (16, 10, 1): stride 6, core 14, so up to three cores hold a voxel along an axis."""
    shape, geometry = (30, 17, 33), (16, 10, 1)
    _stitch(ctx, "linear_35_1000_8", shape, geometry, (0, 0, 0), shape, sub_grid)
    _stitch(ctx, "linear_35_1000_8", shape, geometry, (9, 3, 14), (12, 9, 11), sub_grid)


def test_tile_stitch_u16_rejects_bad_arguments(ctx):
    tf = T.build_transform(TRANSFORM_CFGS["asinh_s32_o35"]).native_struct()
    grid = _native.patch_grid((0, 0, 0), (4, 4, 5), 10, 16)
    d_preds = ctx.alloc(4 * 80 * 16 ** 3).zero()
    out = GuardedView(ctx, np.uint16, 8 * 8 * 8)
    try:
        for n, trim, origin, extent in [(79, 2, (0, 0, 0), (8, 8, 8)), (80, 8, (0, 0, 0), (8, 8, 8)),
                                        (80, 2, (40, 0, 0), (8, 8, 8)), (80, 2, (0, 0, 0), (8, 0, 8)),
                                        (80, -1, (0, 0, 0), (8, 8, 8))]:
            with pytest.raises(ValueError):
                ctx.tile_stitch_u16(tf, d_preds, n, grid, trim, origin, extent, SHAPE, out.ptr)
            ctx.sync()
            out.check_untouched()
    finally:
        out.free()
        d_preds.free()


# ---- predict_store with a model whose output rows do not depend on the batch ------------------------------------
GEO = dict(patch_size=16, overlap=6, trim=2)
CHUNKS = (1, 1, 4, 16, 16)
CFG = TRANSFORM_CFGS["asinh_s32_o35"]


def _smooth(x):
    return x + 0.25 * (F.avg_pool3d(x, 3, 1, 1) - x)


def _files(path):
    out = {}
    for root, _, names in os.walk(path):
        for n in names:
            full = os.path.join(root, n)
            with open(full, "rb") as f:
                out[os.path.relpath(full, path)] = f.read()
    return out


def _stamps(path):
    return {os.path.relpath(os.path.join(r, n), path): (os.stat(os.path.join(r, n)).st_ino,
                                                        os.stat(os.path.join(r, n)).st_mtime_ns)
            for r, _, names in os.walk(path) for n in names}


@pytest.fixture(scope="module")
def smooth_case(tmp_path_factory):
    """The source store, its volume, ``predict`` of it and the store ``write_zarr`` makes of that, computed once."""
    vol, _ = synth_volume(SHAPE, as_u16=True)
    base = tmp_path_factory.mktemp("predict-store")
    src, whole = str(base / "src"), str(base / "whole")
    chunk_store.write_zarr(vol, src, CHUNKS)
    transform = T.build_transform(CFG)
    want = predict(vol, _smooth, transform, batch_size=7, verbose=False, **GEO)
    # the yardstick: the numpy tiling around the same callable
    starts = stitch_pyref.patch_starts(SHAPE, 16, 6)
    inputs = stitch_pyref.gather_patches(vol, CFG, 16, starts)
    with torch.no_grad():
        preds = _smooth(torch.from_numpy(inputs)[:, None].cuda())[:, 0].cpu().numpy()
    np.testing.assert_array_equal(want, stitch_pyref.stitch(preds, starts, SHAPE, 2, CFG))
    ratio = chunk_store.write_zarr(want, whole, CHUNKS, attributes={"k": "v"})
    want.setflags(write=False)
    return src, vol, transform, want, whole, ratio


def test_predict_store_equals_predict_then_write_zarr(smooth_case, tmp_path):
    src, vol, transform, want, whole, want_ratio = smooth_case
    before, stamps = _files(src), _stamps(src)
    files = _files(whole)
    n_chunks = 12 * 3 * 4
    assert len(files) == n_chunks + 1
    seen = []
    for name, budget in [("default", None), ("one-chunk", 1), ("between", 600_000)]:
        dst, stats = str(tmp_path / name), {}
        kw = {} if budget is None else {"budget_bytes": budget}
        ratio = predict_store(src if budget != 1 else chunk_store.open_zarr(src), dst, _smooth, transform, batch_size=7,
                              verbose=False, attributes={"k": "v"}, stats=stats, **GEO, **kw)
        seen.append(stats["bricks"])
        assert stats["patches_unique"] == 80 and stats["patches_run"] >= 80 and stats["largest_alloc"] > 0
        assert set(stats["seconds"]) == {"read", "gather", "forward", "stitch", "scatter", "encode", "files_write"}
        np.testing.assert_array_equal(chunk_store.read_zarr(dst)[0, 0], want)
        assert _files(dst) == files and ratio == want_ratio
        if budget is None:
            assert stats["bricks"] == 1 and stats["patches_run"] == 80
    assert seen[0] == 1 and seen[1] == n_chunks and 1 < seen[2] < n_chunks
    assert _files(src) == before and _stamps(src) == stamps


def test_predict_store_without_a_single_patch(tmp_path):
    """(20, 18, 6): x <= overlap, so no patch exists and every voxel is inverse(0)."""
    shape = (20, 18, 6)
    vol, _ = synth_volume(shape, as_u16=True)
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    chunk_store.write_zarr(vol, src, (1, 1, 8, 8, 8))
    stats = {}
    predict_store(src, dst, _smooth, T.build_transform(CFG), verbose=False, stats=stats, budget_bytes=40_000, **GEO)
    assert stats["patches_run"] == stats["patches_unique"] == 0 and stats["bricks"] > 1
    want = stitch_pyref.stitch(np.zeros((0, 16, 16, 16), F32), [], shape, 2, CFG)
    np.testing.assert_array_equal(chunk_store.read_zarr(dst)[0, 0], want)
    np.testing.assert_array_equal(predict(vol, _smooth, T.build_transform(CFG), verbose=False, **GEO), want)


def test_predict_store_bounded_codec(smooth_case, tmp_path):
    src, vol, transform, want, _, _ = smooth_case
    dst = str(tmp_path / "dst")
    predict_store(src, dst, _smooth, transform, batch_size=7, verbose=False, chunks=(1, 1, 8, 16, 16),
                  codec=BoundedDctCodec(4), budget_bytes=600_000, **GEO)
    blobs = wref.host_blobs(np.asarray(want), (8, 16, 16), "dctq")
    files = _files(dst)
    assert len(files) == len(blobs) + 1
    assert all(files[chunk_store.chunk_key(*idx)] == b for idx, b in blobs.items())


# ---- predict_store with the real U-Net ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet_case(tmp_path_factory):
    torch.manual_seed(0)
    model = UNet(width_multiplier=1).cuda().eval()
    vol, _ = synth_volume((70, 120, 64), as_u16=True)          # 2 x 3 x 1 patches, the last y patch padded
    src = str(tmp_path_factory.mktemp("predict-unet") / "src")
    chunk_store.write_zarr(vol, src, (1, 1, 32, 32, 32))
    return model, vol, src, T.build_transform(CFG)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_predict_store_unet(unet_case, tmp_path, precision):
    """The yardstick for batch sensitivity is ``predict`` itself: d0 = max |predict(batch_size=4) -
    predict(batch_size=3)| in counts, and predict_store may differ from predict(batch_size=4) by max(d0, 1).
    Observed on an MI355X: d0 = 0 (fp32) and 1164 (fp16), and a difference of 0 counts for both --
    here every batch of both routes is a full batch of 4 -- so the assertion is tightened to ``array_equal``; d0 and
    the difference are printed."""
    model, vol, src, transform = unet_case
    a = predict(vol, model, transform, batch_size=4, verbose=False, precision=precision).astype(np.int32)
    b = predict(vol, model, transform, batch_size=3, verbose=False, precision=precision).astype(np.int32)
    d0 = int(np.abs(a - b).max())
    stats = {}
    dst = str(tmp_path / "dst")
    predict_store(src, dst, model, transform, batch_size=4, verbose=False, precision=precision,
                  budget_bytes=12 << 20, stats=stats)
    got = chunk_store.read_zarr(dst)[0, 0].astype(np.int32)
    diff = int(np.abs(got - a).max())
    print(f"predict_store unet {precision}: d0={d0} diff={diff} bricks={stats['bricks']} "
          f"patches_run={stats['patches_run']} differing={int(np.count_nonzero(got != a))}")
    assert stats["bricks"] >= 2 and stats["patches_unique"] == 6
    assert len(np.unique(a)) > 100
    assert diff <= max(d0, 1)
    np.testing.assert_array_equal(got, a)
