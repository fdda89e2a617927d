"""Pyramid levels of a stored LABEL volume, out of core: ``downsample_label_store`` makes one coarser
level of an ``exac-labels`` store as a store of its own, ``pyramid_label_store`` a multiscale group of them,
``downsample_label_volume`` is the in-memory twin.  ``store_pyramid`` does the same for uint16 volumes; the reference's
``write_ome_zarr`` (utils/img_util.py:804-895) reduces with ``windowed_mode``, the one reduction that keeps an id an id.

The rule, all integer and exact.  The geometry is ``store_pyramid``'s: ``factors = (fz, fy, fx)``, each 1 or 2, one at
least 2; level voxel ``(z, y, x)`` reduces the source voxels ``[z fz, min(nz, (z + 1) fz)) x ...``; ``edge="crop"``
gives ``n // f`` voxels per axis, ``"partial"`` ``ceil(n / f)``.  The values are uint32 or uint64 ids, compared as
unsigned integers, and the level has the source's dtype.  ``zeros="count"``: the most frequent value among the voxels
present, of equally frequent values the smallest -- 0 is a value like any other (the uint16 ``"mode"`` on wider
values).  ``zeros="ignore"``: the most frequent NON-ZERO value, of equally frequent ones the smallest; 0 only where
every voxel present is 0 -- the "sparse" mode of segmentation pyramids, under which a neurite one voxel thin does not
vanish at the first level.  There is no mean and no maximum of ids.  Parity with ``xarray_multiscale.windowed_mode``
is not pinned by a test (the library is not a dependency of the tests); ``zeros="ignore"`` has no counterpart in the
reference.

A level voxel depends on its own window only, so a brick of whole destination chunks read with the source voxels under
it gives the whole-volume level exactly.  Per brick: one region read straight from the coded chunks, one kernel launch
(``exabm4d_downsample_box_labels_dev``, ``csrc/label_downsample_kernels.hip``), ``LabelCodec.encode_device``, and the
chunk files.
"""
import json
import os
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_compare, store_pyramid

ZEROS = tuple(_native.LABEL_ZEROS)
GROUP_TYPES = {"count": "mode", "ignore": "mode_nonzero"}      # ``"type"`` of the group document per ``zeros``
_DTYPES = {4: np.dtype(np.uint32), 8: np.dtype(np.uint64)}


# ---- argument checks and the plan -----------------------------------------------------------------------------------
def _check_rule(who, factors, edge, zeros):
    if not isinstance(edge, str) or edge not in _native.DS_EDGES:
        raise ValueError("%s: edge must be one of %s" % (who, ", ".join(store_pyramid.EDGES)))
    if not isinstance(zeros, str) or zeros not in _native.LABEL_ZEROS:
        raise ValueError("%s: zeros must be one of %s" % (who, ", ".join(ZEROS)))
    return store_pyramid._check_factors(who, factors)


def _check_budget(who, budget_bytes):
    if isinstance(budget_bytes, (bool, float, str)) or budget_bytes is None or int(budget_bytes) < 1:
        raise ValueError("%s: budget_bytes must be a positive integer" % who)
    return int(budget_bytes)


def _open_labels(who, src, index):
    """``src`` -- a path or a ``LabelArray`` -- as a ``LabelArray`` opened for device ``index``."""
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.store_labels import LabelArray
    if isinstance(src, (str, os.PathLike)):
        try:
            src = chunk_store.open_zarr(src, device=index)
        except NotImplementedError as e:
            raise ValueError("%s: src must be a label store (%s)" % (who, e)) from None
    if not isinstance(src, LabelArray):
        raise ValueError("%s: src is the path of an exac-labels store or a LabelArray (uint32 / uint64 ids)" % who)
    if int(src.device if src.device is not None else _native.default_device()) != index:
        raise ValueError("%s: src was opened for another device than %d, the one used here" % (who, index))
    return src


def _same_window(b0, bd, dim):
    return b0, bd


def _plan(who, shape, factors, edge, chunks_zyx, budget_bytes, typesize):
    """``plan_label_downsample``; with ``factors`` None the plan of a copy: the level is the source and a brick's window
    is the brick, which the encoder reads where the reader left it."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("%s: shape and chunks are three positive sizes each" % who)
    if typesize not in _DTYPES:
        raise ValueError("%s: typesize is 4 (uint32) or 8 (uint64)" % who)
    budget, ts = _check_budget(who, budget_bytes), int(typesize)
    if factors is None:
        return shape, store_compare.plan_bricks(shape, chunk, budget, 1, _same_window, ts + 1, ts)
    level = store_pyramid.level_shape(shape, factors, edge)
    if min(level) < 1:
        raise ValueError("%s: a volume of %s has no level under factors %s and edge %r" % (who, shape, factors, edge))
    windows = [store_pyramid.source_window(k, n) for k, n in zip(factors, shape)]
    return level, store_compare.plan_bricks(level, chunk, budget, 1, windows, ts + ts + 1, ts)


def plan_label_downsample(shape, factors, edge, chunks_zyx, budget_bytes, typesize):
    """``(level_shape, bricks)`` of downsampling a label volume of ``shape`` (z, y, x) and elements of ``typesize``
    bytes by ``factors`` into a store with chunks of ``chunks_zyx``.  The bricks (``store_compare.Brick``, raster order)
    are boxes of whole destination chunks in LEVEL coordinates that partition the level, grown as
    ``store_compare.plan_compare`` grows them; ``win_origin`` / ``win_extent`` are the source voxels under a brick, in
    SOURCE coordinates.  A brick costs its source window at ``typesize`` bytes a voxel, the reader's share of the
    budget for the coded chunks it holds, and per level voxel ``typesize`` for the dense brick plus ``typesize + 1`` for
    the encoder's bound (``store_segment.segment_brick_bytes`` counts the two the same way).  A brick of a single chunk
    is accepted whatever it costs."""
    f = _check_rule("plan_label_downsample", factors, edge, "count")
    return _plan("plan_label_downsample", shape, f, edge, chunks_zyx, budget_bytes, typesize)


# ---- one level --------------------------------------------------------------------------------------------------------
def _run_bricks(who, arr, dst_path, shape, bricks, chunks, factors, edge, zeros, attributes, budget, index, stats):
    """The brick loop of one destination store: read, reduce (left out with ``factors`` None: a copy at other chunks),
    encode, commit.  Returns the bytes written."""
    from aind_exaspim_image_compression.utils import chunk_store, store_windows, store_write
    from aind_exaspim_image_compression.utils.label_codec import LabelCodec
    ts = int(arr.dtype.itemsize)
    src_shape = tuple(int(s) for s in arr.shape[2:])
    ctx = _native.context(index)
    codec = LabelCodec(ts, device=index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    chunk3 = tuple(int(c) for c in chunks[2:])
    clock = store_windows.PhaseClock(("read", "reduce", "encode", "files_write"), stats is not None, ctx.sync)
    seconds = clock.seconds
    voxels_read = most = written = 0
    with store_windows.capped_pools([arr], budget):
        for brick in bricks:
            nvox = int(np.prod(brick.extent))
            t0 = time.perf_counter()
            win = arr.read_patches([brick.win_origin], brick.win_extent, is_center=False, out="device")
            d_brick = None
            try:
                t1 = clock()
                voxels_read += brick.window_voxels
                if factors is None:
                    d_level = win.buf
                else:
                    d_level = d_brick = ctx.alloc(ts * nvox)
                    most = max(most, ts * brick.window_voxels + ts * nvox)
                    ctx.downsample_box_labels(win.buf, arr.dtype, src_shape, brick.win_origin, brick.win_extent,
                                              brick.origin, brick.extent, factors, edge, zeros, out=d_brick)
                t2 = clock()
                if factors is not None:
                    win.free()                           # (freeing a buffer waits for the stream)
                most = max(most, ts * nvox + _native.label_encode_bound(ts, brick.extent, codec._chunk(
                    brick.extent, chunk3)))
                enc = codec.encode_device(ctx, d_level, brick.extent, chunk3)
                t3 = time.perf_counter()
                written += store_write.commit_coded_brick(who, out, brick, chunk3, enc)
                seconds["read"] += t1 - t0
                seconds["reduce"] += t2 - t1
                seconds["encode"] += t3 - t2
                seconds["files_write"] += time.perf_counter() - t3
            finally:
                win.free()
                if d_brick is not None:
                    d_brick.free()
    if stats is not None:
        stats.update(seconds=seconds, bricks=len(bricks), voxels_read=voxels_read, largest_alloc=most)
    return written


def downsample_label_store(src, dst_path, factors=(2, 2, 2), edge="crop", zeros="count", chunks=None, attributes=None,
                           budget_bytes=4 << 30, device=None, stats=None):
    """One coarser level of the stored label volume ``src`` as a label store of its own, without ever holding the
    volume: ``dst_path`` is, chunk file for chunk file, ``write_zarr(level, dst_path, chunks, codec=LabelCodec(ts))`` of
    the level that the rule of the module docstring makes of the whole array, whatever the brick plan.

    ``src``: a path or a ``LabelArray`` opened for the device used here; anything else, a uint16 store included, is a
    ``ValueError``.  The destination is made with ``create_zarr`` (``chunks``: default the source's;
    ``LabelCodec`` of the source's typesize; ``attributes``).  Bricks are boxes of whole destination chunks
    (``plan_label_downsample``, at most ``budget_bytes`` of device memory each; a single chunk is taken whatever it
    costs).  Per brick: one region read of the source voxels under it, straight from the coded chunks, that stays on
    the device; one kernel launch into a dense brick; ``LabelCodec.encode_device``; the chunk files, each replaced
    atomically.

    Returns ``{"shape", "n", "cratio"}``: the level's shape, its voxels, raw bytes / stored bytes.  ``stats`` (a dict)
    receives ``seconds`` per phase (read, reduce, encode, files_write; the stream is synchronised around the phases only
    when ``stats`` is given), ``bricks``, ``voxels_read`` and ``largest_alloc``, the most device bytes held here at one
    time (the reader's coded chunks apart)."""
    from aind_exaspim_image_compression.utils import store_windows
    who = "downsample_label_store"
    # -- every argument check, before a context exists
    f = _check_rule(who, factors, edge, zeros)
    budget = _check_budget(who, budget_bytes)
    chunks = store_windows.check_chunks(chunks)
    index = int(device) if device is not None else _native.default_device()
    arr = _open_labels(who, src, index)
    ts = int(arr.dtype.itemsize)
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    shape, bricks = _plan(who, arr.shape[2:], f, edge, chunks[2:], budget, ts)
    written = _run_bricks(who, arr, dst_path, shape, bricks, chunks, f, edge, zeros, attributes, budget, index, stats)
    n = shape[0] * shape[1] * shape[2]
    return {"shape": shape, "n": n, "cratio": ts * n / written}


def downsample_label_volume(vol, factors=(2, 2, 2), edge="crop", zeros="count", device=None):
    """``downsample_label_store`` for a 3-D uint32 / uint64 array in memory: the level as a host array of the same
    dtype.  One upload, one launch, one download."""
    vol = np.asarray(vol)
    if vol.dtype not in _DTYPES.values() or vol.ndim != 3 or 0 in vol.shape:
        raise ValueError("downsample_label_volume: vol is a 3-D uint32 or uint64 array without an empty axis")
    f = _check_rule("downsample_label_volume", factors, edge, zeros)
    src_shape = tuple(int(s) for s in vol.shape)
    shape = store_pyramid.level_shape(src_shape, f, edge)
    if min(shape) < 1:
        raise ValueError("downsample_label_volume: a volume of %s has no level under factors %s and edge %r"
                         % (src_shape, f, edge))
    ctx = _native.context(device)
    d_vol = d_out = None
    try:
        d_vol = ctx.to_device(np.ascontiguousarray(vol))
        d_out = ctx.alloc(vol.dtype.itemsize * int(np.prod(shape)))
        ctx.downsample_box_labels(d_vol, vol.dtype, src_shape, (0, 0, 0), src_shape, (0, 0, 0), shape, f, edge, zeros,
                                  out=d_out)
        return d_out.download(shape, vol.dtype)
    finally:
        for buf in (d_vol, d_out):
            if buf is not None:
                buf.free()


# ---- the multiscale group -------------------------------------------------------------------------------------------
def pyramid_label_store(src, dst_path, n_levels, factors=(2, 2, 2), edge="crop", zeros="count", chunks=None,
                        voxel_size=(748, 748, 1000), scale=None, translation=None, spatial_unit="nanometer",
                        budget_bytes=4 << 30, device=None, stats=None):
    """The stored label volume ``src`` as a multiscale group of ``n_levels`` label stores, store to store: ``<dst>/0`` is
    the source at ``chunks`` (chunk file for chunk file ``write_zarr`` of the source array; the brick loop with the
    reduction left out), ``<dst>/k`` is ``downsample_label_store(<dst>/k-1, ...)`` -- each level from the level before
    it -- and, written last, ``<dst>/zarr.json`` is ``store_pyramid.group_document`` of
    ``store_pyramid.level_transforms`` with the type ``"mode"`` (``zeros="count"``) or ``"mode_nonzero"``
    (``"ignore"``): a group without it is incomplete, and an old one is removed first.
    ``store_pyramid.open_multiscale`` opens the result and hands back ``LabelArray``s.

    ``factors``: one triple for every step, or ``n_levels - 1`` triples, one per step.  ``chunks`` (default the
    source's) hold for every level.  Every level's shape is worked out first: a level that would get an empty axis
    raises ``ValueError`` before anything is written.  Returns ``{"shapes", "cratios", "transforms"}`` per level;
    ``stats`` (a dict) receives ``levels``, the ``stats`` of each step."""
    from aind_exaspim_image_compression.utils import store_windows
    who = "pyramid_label_store"
    # -- every argument check, before a context exists and before anything is written
    steps = store_pyramid._level_factors(n_levels, factors, who)
    _check_rule(who, (2, 2, 2), edge, zeros)
    budget = _check_budget(who, budget_bytes)
    chunks = store_windows.check_chunks(chunks)
    transforms = store_pyramid.level_transforms(steps, voxel_size, scale, translation)
    if not isinstance(spatial_unit, str):
        raise ValueError("%s: spatial_unit is a string" % who)
    index = int(device) if device is not None else _native.default_device()
    arr = _open_labels(who, src, index)
    ts = int(arr.dtype.itemsize)
    shapes = [tuple(int(s) for s in arr.shape[2:])]
    for k, step in enumerate(steps):
        shapes.append(store_pyramid.level_shape(shapes[-1], step, edge))
        if min(shapes[-1]) < 1:
            raise ValueError("%s: level %d of a volume of %s would have the shape %s"
                             % (who, k + 1, shapes[0], shapes[-1]))
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    _, bricks = _plan(who, shapes[0], None, edge, chunks[2:], budget, ts)

    os.makedirs(dst_path, exist_ok=True)
    group_file = os.path.join(dst_path, "zarr.json")
    if os.path.exists(group_file):
        os.remove(group_file)                            # incomplete until it is written again
    per_level, cratios = [], []
    level_stats = {} if stats is not None else None
    written = _run_bricks(who, arr, os.path.join(dst_path, "0"), shapes[0], bricks, chunks, None, edge, zeros, None,
                          budget, index, level_stats)
    cratios.append(ts * int(np.prod(shapes[0])) / written)
    per_level.append(level_stats)
    for k, step in enumerate(steps):
        level_stats = {} if stats is not None else None
        res = downsample_label_store(os.path.join(dst_path, str(k)), os.path.join(dst_path, str(k + 1)), step, edge,
                                     zeros, chunks=chunks, budget_bytes=budget, device=index, stats=level_stats)
        if res["shape"] != shapes[k + 1]:
            raise RuntimeError("%s: level %d came out as %s, not %s" % (who, k + 1, res["shape"], shapes[k + 1]))
        cratios.append(res["cratio"])
        per_level.append(level_stats)
    with open(group_file, "w") as fh:                    # last: a group without it is incomplete
        json.dump(store_pyramid.group_document(transforms, GROUP_TYPES[zeros], spatial_unit), fh, indent=1)
    if stats is not None:
        stats.update(levels=per_level)
    return {"shapes": shapes, "cratios": cratios, "transforms": transforms}
