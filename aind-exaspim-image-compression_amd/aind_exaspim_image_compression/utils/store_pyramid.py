"""Pyramid levels of a stored volume, out of core: ``downsample_store`` makes one coarser level of a
store as a store of its own, ``pyramid_store`` a multiscale group of them -- what the reference's ``write_ome_zarr``
(utils/img_util.py:804-895) makes of a volume in memory with ``windowed_mode`` over 2 x 2 x 2 windows, each level from
the level before it --, ``downsample_volume`` is the in-memory twin.

The rule, all integer and exact.  ``factors = (fz, fy, fx)``, each 1 or 2, one at least 2.  Level voxel ``(z, y, x)``
reduces the source voxels ``[z fz, min(nz, (z + 1) fz)) x ...``: 1, 2, 4 or 8 of them.  ``edge="crop"``: the level has
``n // f`` voxels per axis and no window is ever cut; ``edge="partial"``: ``ceil(n / f)``, and the last window of an
axis may be cut.  ``method="mode"``: the most frequent value, of values equally frequent the smallest; ``"mean"``:
``sum / count`` rounded half to even; ``"max"``: the largest value (a mask's "any voxel set").  A level voxel depends
on its own window only, so a brick of whole destination chunks read with the source voxels under it -- no halo -- gives
the whole-volume level exactly.  Per brick one kernel launch (``exabm4d_downsample_box_u16_dev``,
``csrc/downsample_kernels.hip``).
"""
import json
import os
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_compare
from aind_exaspim_image_compression.utils.store_predict import BRICK_BYTES, POOL_BYTES

METHODS = tuple(_native.DS_METHODS)
EDGES = tuple(_native.DS_EDGES)
GROUP_NOTE = ("levels are EXAC chunk stores (aind-exaspim-image-compression_amd, DESIGN.md 5.21); open with "
              "utils.chunk_store.open_multiscale")


# ---- argument checks and shapes -------------------------------------------------------------------------------------
def _check_factors(who, factors):
    try:
        f = tuple(factors)
        ok = len(f) == 3 and all(not isinstance(v, (bool, float)) and int(v) == v and int(v) in (1, 2) for v in f)
    except (TypeError, ValueError):
        ok = False
    if not ok or max(f) != 2:
        raise ValueError("%s: factors are (fz, fy, fx), each 1 or 2 and one at least 2" % who)
    return tuple(int(v) for v in f)


def _check_rule(who, factors, method, edge):
    if not isinstance(method, str) or method not in _native.DS_METHODS:
        raise ValueError("%s: method must be one of %s" % (who, ", ".join(METHODS)))
    if not isinstance(edge, str) or edge not in _native.DS_EDGES:
        raise ValueError("%s: edge must be one of %s" % (who, ", ".join(EDGES)))
    return _check_factors(who, factors)


def level_shape(shape, factors, edge="crop"):
    """The (z, y, x) shape of the level that ``factors`` make of a volume of ``shape``: ``n // f`` per axis under
    ``edge="crop"`` (an axis may come out empty), ``ceil(n / f)`` under ``"partial"``."""
    if edge not in _native.DS_EDGES:
        raise ValueError("level_shape: edge must be one of %s" % ", ".join(EDGES))
    f = _check_factors("level_shape", factors)
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("level_shape: shape is three positive sizes")
    return tuple(n // k if edge == "crop" else -(-n // k) for n, k in zip(shape, f))


def source_window(factor, source_dim):
    """``axis_window`` of ``store_compare.plan_bricks`` for one axis of a level: the level voxels ``[b0, b0 + bd)`` read
    the source voxels ``[b0 f, min(n, (b0 + bd) f))``."""
    def axis_window(b0, bd, dim):
        lo = b0 * factor
        return lo, min(source_dim, (b0 + bd) * factor) - lo
    return axis_window


def plan_downsample(shape, factors, edge, chunks_zyx, budget_bytes):
    """``(level_shape, bricks)`` of downsampling a volume of ``shape`` (z, y, x) by ``factors`` into a store with chunks
    of ``chunks_zyx``.  The bricks (``store_compare.Brick``, raster order) are boxes of whole destination chunks in
    LEVEL coordinates that partition the level, grown as ``store_compare.plan_compare`` grows them; ``win_origin`` /
    ``win_extent`` are the source voxels under a brick, in SOURCE coordinates.  A brick costs its source window at
    ``WINDOW_BYTES`` a voxel as it is held (read in z slabs of about a destination chunk), the reader's pool of decoded
    chunks (``budget_bytes // READER_SHARE``), and per level voxel the dense brick and the destination pool with its
    coded streams.  A brick of a single chunk is accepted whatever it costs."""
    f = _check_rule("plan_downsample", factors, "mode", edge)
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    budget = int(budget_bytes)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_downsample: shape and chunks are three positive sizes each")
    if budget < 1:
        raise ValueError("plan_downsample: budget_bytes >= 1")
    level = level_shape(shape, f, edge)
    if min(level) < 1:
        raise ValueError("plan_downsample: a volume of %s has no level under factors %s and edge %r" % (shape, f, edge))
    windows = [source_window(k, n) for k, n in zip(f, shape)]
    return level, store_compare.plan_bricks(level, chunk, budget, 1, windows, BRICK_BYTES + POOL_BYTES)


# ---- one level --------------------------------------------------------------------------------------------------------
def downsample_store(src, dst_path, factors=(2, 2, 2), method="mode", edge="crop", chunks=None, codec=None,
                     attributes=None, budget_bytes=4 << 30, device=None, stats=None):
    """One coarser level of the stored uint16 volume ``src`` as a store of its own, without ever holding the volume:
    ``dst_path`` is, chunk file for chunk file, ``write_zarr(level, dst_path, chunks, codec)`` of the level that the
    rule of the module docstring makes of ``read_zarr(src)[0, 0]``, whatever the brick plan.

    ``src``: a path or a ``StoredArray`` opened for the device used here -- a volume, or a mask store (``"max"``:
    the level of a mask is a mask, with its value).  The destination is made with ``create_zarr`` (``chunks``: default
    the source's; ``codec``: any codec it takes, default ``ExacCodec(2)``; ``attributes``).  Bricks are boxes of whole
    destination chunks (``plan_downsample``, at most ``budget_bytes`` of device memory each; a single chunk is taken
    whatever it costs).  Per brick: one region read of the source voxels under it that stays on the device, one kernel
    launch into a dense brick, a scatter into the pool of destination chunks, which is coded and committed.

    Returns ``{"shape", "n", "cratio"}``: the level's shape, its voxels, raw bytes / stored bytes.  ``stats`` (a dict)
    receives ``seconds`` per phase (read, reduce, scatter, encode, files_write; the stream is synchronised around the
    phases only when ``stats`` is given), ``bricks``, ``voxels_read`` and ``largest_alloc``, the most device bytes held
    here at one time."""
    from aind_exaspim_image_compression.utils import chunk_store, store_windows, store_write
    # -- every argument check, before a context exists
    f = _check_rule("downsample_store", factors, method, edge)
    chunks, codec, budget = store_windows.check_store_args("downsample_store", chunks, codec, budget_bytes)
    index = int(device) if device is not None else _native.default_device()
    (arr,) = store_windows.open_u16_stores("downsample_store", (("src", src),), index)
    src_shape = tuple(int(s) for s in arr.shape[2:])
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    shape, bricks = plan_downsample(src_shape, f, edge, chunks[2:], budget)

    ctx = _native.context(index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    source = store_windows.StoreWindows([arr], int(chunks[2]))
    clock = store_windows.PhaseClock(("read", "reduce", "scatter", "encode", "files_write"), stats is not None,
                                     ctx.sync)
    seconds = clock.seconds
    voxels_read, most = 0, 0
    with store_windows.BrickSink("downsample_store", out, ctx, shape, chunks) as sink, \
            store_windows.capped_pools([arr], budget):
        for brick in bricks:
            nvox = int(np.prod(brick.extent))
            group = sink.pool([brick.origin], [brick.extent])
            t0 = time.perf_counter()
            wins, dims = source.read(brick.win_origin, brick.win_extent)
            try:
                t1 = clock()
                with ctx.alloc(2 * nvox) as d_brick:
                    most = max(most, 2 * int(np.prod(dims)) + 2 * nvox)
                    ctx.downsample_box_u16(wins[0], src_shape, brick.win_origin, dims, brick.origin, brick.extent,
                                           f, method, edge, out_u16=d_brick)
                    t2 = clock()
                    source.release(wins)                 # (freeing a buffer waits for the stream)
                    voxels_read += brick.window_voxels
                    with group as pool:
                        most = max(most, 2 * nvox + 2 * pool.g.pool_elems)
                        pool.scatter(d_brick, nvox, np.uint16, store_write.box_records([brick.origin], brick.extent))
                        t3 = clock()
                        d_brick.free()
                        seconds["read"] += t1 - t0
                        seconds["reduce"] += t2 - t1
                        seconds["scatter"] += t3 - t2
                        pool.commit()
            finally:
                source.release(wins)
    n = shape[0] * shape[1] * shape[2]
    if stats is not None:
        stats.update(sink.finish(seconds), seconds=seconds, bricks=len(bricks), voxels_read=voxels_read,
                     largest_alloc=most)
    return {"shape": shape, "n": n, "cratio": 2 * n / sink.written}


def downsample_volume(vol, factors=(2, 2, 2), method="mode", edge="crop", device=None):
    """``downsample_store`` for a 3-D uint16 array in memory: the level as a host uint16 array.  The array is uploaded
    once and reduced as one brick."""
    vol = np.asarray(vol)
    if vol.dtype != np.uint16 or vol.ndim != 3 or 0 in vol.shape:
        raise ValueError("downsample_volume: vol is a 3-D uint16 array without an empty axis")
    f = _check_rule("downsample_volume", factors, method, edge)
    src_shape = tuple(int(s) for s in vol.shape)
    shape = level_shape(src_shape, f, edge)
    if min(shape) < 1:
        raise ValueError("downsample_volume: a volume of %s has no level under factors %s and edge %r"
                         % (src_shape, f, edge))
    ctx = _native.context(device)
    d_vol = d_out = None
    try:
        d_vol = ctx.to_device(np.ascontiguousarray(vol))
        d_out = ctx.alloc(2 * int(np.prod(shape)))
        ctx.downsample_box_u16(d_vol, src_shape, (0, 0, 0), src_shape, (0, 0, 0), shape, f, method, edge, out_u16=d_out)
        return d_out.download(shape, np.uint16)
    finally:
        for buf in (d_vol, d_out):
            if buf is not None:
                buf.free()


# ---- the multiscale group -------------------------------------------------------------------------------------------
def _five(name, values):
    try:
        v = np.asarray(values, dtype=float)
    except (TypeError, ValueError):
        v = np.zeros(0)
    if v.shape != (5,) or not np.isfinite(v).all():
        raise ValueError("%s must have five values in (t, c, z, y, x) order" % name)
    return v


def _level_factors(n_levels, factors, who="pyramid_store"):
    """``n_levels - 1`` checked triples from one triple or from one per step."""
    if isinstance(n_levels, (bool, float)) or int(n_levels) != n_levels or n_levels < 1:
        raise ValueError("%s: n_levels must be an integer >= 1" % who)
    try:
        nested = len(factors) > 0 and all(hasattr(t, "__len__") for t in factors)
    except TypeError:
        nested = False
    if not nested:
        return [_check_factors(who, factors)] * (int(n_levels) - 1)
    if len(factors) != n_levels - 1:
        raise ValueError("%s: factors are one triple, or n_levels - 1 triples, one per step" % who)
    return [_check_factors(who, t) for t in factors]


def level_transforms(steps, voxel_size=(748, 748, 1000), scale=None, translation=None):
    """``[(scale, translation), ...]`` (five values each, t c z y x) of level 0 and of the level after each of
    ``steps`` (factor triples), as the reference states them (utils/img_util.py:840-877): the base scale is ``[1, 1,
    *reversed(voxel_size)]`` unless ``scale`` is given; ``scale_k`` = the base scale times the cumulative factors, and
    ``translation_k = base_translation + (scale_k - base_scale) / 2`` -- a coarser voxel's centre lies half the increase
    in voxel size further in."""
    if scale is None:
        try:
            ok = len(voxel_size) == 3
        except TypeError:
            ok = False
        if not ok:
            raise ValueError("voxel_size must have three values in (x, y, z) order")
    base_scale = _five("scale", scale if scale is not None else [1, 1, *reversed(voxel_size)])
    base_translation = _five("translation", translation if translation is not None else np.zeros(5))
    out, cumulative = [], np.ones(5)
    for step in [None] + list(steps):
        if step is not None:
            cumulative = cumulative * np.array([1, 1, *step], dtype=float)
        level_scale = base_scale * cumulative
        out.append((level_scale.tolist(), (base_translation + (level_scale - base_scale) / 2).tolist()))
    return out


def group_document(transforms, method, spatial_unit="nanometer"):
    """The ``zarr.json`` of a multiscale group: a Zarr v3 group whose ``attributes.ome.multiscales`` names the levels
    ``"0", "1", ...`` with a scale and a translation each, under the reference's five axes; ``"type"`` is the
    method."""
    datasets = [{"path": str(k), "coordinateTransformations": [{"type": "scale", "scale": list(s)},
                                                                {"type": "translation", "translation": list(t)}]}
                for k, (s, t) in enumerate(transforms)]
    axes = [{"name": "t", "type": "time", "unit": "millisecond"}, {"name": "c", "type": "channel"},
            {"name": "z", "type": "space", "unit": spatial_unit}, {"name": "y", "type": "space", "unit": spatial_unit},
            {"name": "x", "type": "space", "unit": spatial_unit}]
    return {"zarr_format": 3, "node_type": "group",
            "attributes": {"ome": {"version": "0.5",
                                   "multiscales": [{"name": "/", "axes": axes, "datasets": datasets, "type": method}]},
                           "exac_note": GROUP_NOTE}}


def pyramid_store(src, dst_path, n_levels, factors=(2, 2, 2), method="mode", edge="crop", chunks=None, codec=None,
                  voxel_size=(748, 748, 1000), scale=None, translation=None, spatial_unit="nanometer",
                  budget_bytes=4 << 30, device=None, stats=None):
    """The stored uint16 volume ``src`` as a multiscale group of ``n_levels`` levels, store to store: ``<dst>/0`` is
    ``recode_store(src, ...)``, ``<dst>/k`` is ``downsample_store(<dst>/k-1, ...)`` -- each level from the level before
    it, as the reference chains them -- and, written last, ``<dst>/zarr.json`` is the group document
    (``group_document`` of ``level_transforms``): a group without it is incomplete.

    ``factors``: one triple for every step, or ``n_levels - 1`` triples, one per step.  ``chunks`` (default the
    source's) and ``codec`` (default ``ExacCodec(2)``) hold for every level.  Every level's shape is worked out first:
    a level that would get an empty axis raises ``ValueError`` before anything is written.  Returns ``{"shapes",
    "cratios", "transforms"}`` per level; ``stats`` (a dict) receives ``levels``, the ``stats`` of each step."""
    from aind_exaspim_image_compression.utils import store_recode, store_windows
    # -- every argument check, before a context exists and before anything is written
    steps = _level_factors(n_levels, factors)
    _check_rule("pyramid_store", (2, 2, 2), method, edge)
    chunks, codec, budget = store_windows.check_store_args("pyramid_store", chunks, codec, budget_bytes)
    transforms = level_transforms(steps, voxel_size, scale, translation)
    if not isinstance(spatial_unit, str):
        raise ValueError("pyramid_store: spatial_unit is a string")
    index = int(device) if device is not None else _native.default_device()
    (arr,) = store_windows.open_u16_stores("pyramid_store", (("src", src),), index)
    shapes = [tuple(int(s) for s in arr.shape[2:])]
    for k, step in enumerate(steps):
        shapes.append(level_shape(shapes[-1], step, edge))
        if min(shapes[-1]) < 1:
            raise ValueError("pyramid_store: level %d of a volume of %s would have the shape %s"
                             % (k + 1, shapes[0], shapes[-1]))
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)

    os.makedirs(dst_path, exist_ok=True)
    group_file = os.path.join(dst_path, "zarr.json")
    if os.path.exists(group_file):
        os.remove(group_file)                            # incomplete until it is written again
    per_level, cratios = [], []
    level_stats = {} if stats is not None else None
    cratios.append(store_recode.recode_store(arr, os.path.join(dst_path, "0"), codec=codec, chunks=chunks,
                                             budget_bytes=budget, device=index, stats=level_stats))
    per_level.append(level_stats)
    for k, step in enumerate(steps):
        level_stats = {} if stats is not None else None
        res = downsample_store(os.path.join(dst_path, str(k)), os.path.join(dst_path, str(k + 1)), step, method, edge,
                               chunks=chunks, codec=codec, budget_bytes=budget, device=index, stats=level_stats)
        if res["shape"] != shapes[k + 1]:
            raise RuntimeError("pyramid_store: level %d came out as %s, not %s" % (k + 1, res["shape"], shapes[k + 1]))
        cratios.append(res["cratio"])
        per_level.append(level_stats)
    with open(group_file, "w") as fh:                    # last: a group without it is incomplete
        json.dump(group_document(transforms, method, spatial_unit), fh, indent=1)
    if stats is not None:
        stats.update(levels=per_level)
    return {"shapes": shapes, "cratios": cratios, "transforms": transforms}


def open_multiscale(path, device=None):
    """A multiscale group (``pyramid_store``) -> ``(levels, transforms)``: the ``StoredArray`` of every level in order
    and its ``(scale, translation)`` pair.  Reads the ``zarr.json`` documents only; ``ValueError`` for a directory
    that is no such group."""
    from aind_exaspim_image_compression.utils import chunk_store
    with open(os.path.join(path, "zarr.json")) as fh:
        doc = json.load(fh)
    try:
        if doc["zarr_format"] != 3 or doc["node_type"] != "group":
            raise ValueError("not a Zarr v3 group")
        (multiscale,) = doc["attributes"]["ome"]["multiscales"]
        levels, transforms = [], []
        for entry in multiscale["datasets"]:
            found = {t["type"]: t[t["type"]] for t in entry["coordinateTransformations"]}
            transforms.append(([float(v) for v in found["scale"]],
                               [float(v) for v in found.get("translation", [0.0] * 5)]))
            levels.append(chunk_store.open_zarr(os.path.join(path, entry["path"]), device=device))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s holds no multiscale group this reader takes: %s" % (path, e)) from None
    return levels, transforms
