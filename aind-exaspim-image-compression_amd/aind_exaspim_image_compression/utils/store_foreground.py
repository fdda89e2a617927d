"""The foreground mask of a stored volume, out of core: ``foreground_store`` makes
``make_foreground_mask`` of the whole volume store to store, ``foreground_volume`` is its in-memory twin.

Two facts carry it.  The whole-volume threshold follows exactly from the table of the counts that
``utils.noise.measure_store`` makes (``StoreMeasure.foreground_threshold``), and for integer counts ``raw > thr`` is the
integer test ``raw >= cut``.  And ``dilate`` iterations of the 6-neighbour cross with border 0 are one dilation by the L1
ball of radius ``dilate``, cut at the volume's faces: a brick read with a halo of ``dilate`` voxels gives the
whole-volume mask exactly.  Per brick one kernel launch thresholds, packs and dilates
(``exabm4d_foreground_box_u16_dev``, ``csrc/foreground_kernels.hip``).

With ``min_voxels`` the seeds are filtered before the dilation: a seed survives if and only if its
connected component among the seeds of the whole volume has at least ``min_voxels`` voxels.  A halo of ``min_voxels -
1`` voxels more decides that for every seed of a brick exactly as the whole volume would: a smaller component lies
within ``min_voxels - 2`` steps of the seed, whole and connected inside the window; of a larger one the first
``min_voxels`` voxels of a breadth-first walk lie within ``min_voxels - 1`` steps (a step moves at most one voxel per
axis, under 6- and 26-connectivity alike).  ``exabm4d_component_seeds_u16_dev`` (``csrc/component_kernels.hip``) labels
and filters; the mask kernel then runs unchanged on the filtered seeds.
"""
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_compare
from aind_exaspim_image_compression.utils.store_measure import StoreMeasure, cut_of_threshold
from aind_exaspim_image_compression.utils.store_predict import BRICK_BYTES, POOL_BYTES

MAX_DILATE = _native.FG_MAX_RADIUS
MAX_MIN_VOXELS = 64         # of the store path: a brick's halo grows by min_voxels - 1
# what the filter holds per voxel of a window besides the window: three 32-bit arrays of scratch (parents, labels,
# sizes) and the filtered seeds of the brick and its dilation halo at 2 bytes; and the scratch's alignment per brick
COMPONENT_BYTES = 3 * 4 + 2
COMPONENT_FIXED_BYTES = 3 * 256


def halo_window(radius):
    """``axis_window`` of ``store_compare.plan_bricks``: ``[max(0, b0 - radius), min(dim, b0 + bd + radius))``."""
    def axis_window(b0, bd, dim):
        lo = max(0, b0 - radius)
        return lo, min(dim, b0 + bd + radius) - lo
    return axis_window


def _grown(shape, origin, extent, by):
    """(origin, extent) of a box grown by ``by`` voxels per axis and cut at the volume's faces."""
    window = halo_window(by)
    pairs = [window(o, e, n) for o, e, n in zip(origin, extent, shape)]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


def plan_foreground(shape, chunks_zyx, dilate, budget_bytes, min_voxels=0):
    """The bricks (``store_compare.Brick``) of masking a volume of ``shape`` (z, y, x) into a store with chunks of
    ``chunks_zyx``, in raster order: boxes of whole destination chunks that partition the volume, grown as
    ``store_compare.plan_compare`` grows them.  A brick's window is the brick grown by ``dilate`` voxels per axis and
    cut at the volume's faces.  A brick costs its window at 2 bytes a voxel as it is held, the reader's pool of decoded
    chunks (``budget_bytes // READER_SHARE``), and per voxel of the brick the dense mask and the destination pool with
    its coded streams.  A brick of a single chunk is accepted whatever it costs.

    With ``min_voxels`` (0..``MAX_MIN_VOXELS``) the halo is ``dilate + max(0, min_voxels - 1)`` voxels, and from 1 on a
    brick also costs what the component filter holds: ``COMPONENT_BYTES`` per voxel of the window (the scratch of
    ``exabm4d_components_scratch_bytes`` and the filtered seeds) and ``COMPONENT_FIXED_BYTES``."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    dilate, budget = int(dilate), int(budget_bytes)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_foreground: shape and chunks are three positive sizes each")
    if not 0 <= dilate <= MAX_DILATE or budget < 1:
        raise ValueError("plan_foreground: 0 <= dilate <= %d and budget_bytes >= 1" % MAX_DILATE)
    min_voxels = _check_filter_args("plan_foreground", min_voxels, 26, MAX_MIN_VOXELS)
    if min_voxels == 0:
        return store_compare.plan_bricks(shape, chunk, budget, 1, halo_window(dilate), BRICK_BYTES + POOL_BYTES)
    return store_compare.plan_bricks(shape, chunk, budget, 1, halo_window(dilate + min_voxels - 1),
                                     BRICK_BYTES + POOL_BYTES, store_compare.WINDOW_BYTES + COMPONENT_BYTES,
                                     COMPONENT_FIXED_BYTES)


def _check_mask_args(who, k, dilate, threshold, value=1):
    dilate = int(dilate)
    if not 0 <= dilate <= MAX_DILATE:
        raise ValueError("%s: dilate must be 0..%d" % (who, MAX_DILATE))
    if not 1 <= int(value) <= 65535:
        raise ValueError("%s: value must be 1..65535" % who)
    if threshold is not None:
        if not np.isfinite(float(threshold)):
            raise ValueError("%s: threshold must be a finite number of counts" % who)
    elif not np.isfinite(float(k)) or float(k) < 0.0:
        raise ValueError("%s: k must be finite and >= 0" % who)
    return dilate, int(value)


def _check_filter_args(who, min_voxels, connectivity, most=2 ** 31 - 1, least=0):
    if connectivity not in (6, 26):
        raise ValueError("%s: connectivity must be 6 or 26" % who)
    if isinstance(min_voxels, (bool, float)) or int(min_voxels) != min_voxels or not least <= min_voxels <= most:
        raise ValueError("%s: min_voxels must be an integer %d..%d" % (who, least, most))
    return int(min_voxels)


def foreground_store(src, dst_path, k=6.0, dilate=1, threshold=None, measure=None, value=1, chunks=None, codec=None,
                     attributes=None, budget_bytes=4 << 30, device=None, stats=None, min_voxels=0, connectivity=26):
    """The foreground mask of the stored uint16 volume ``src`` as a store of its own, without ever holding the volume:
    ``dst_path`` is, chunk file for chunk file, ``write_zarr((make_foreground_mask(read_zarr(src)[0, 0], k, dilate) *
    value).astype(uint16), dst_path, chunks, codec)`` -- a mask store (uint16, non-zero = foreground) as
    ``measure_store(mask=)``, ``compare_stores(mask=)`` and ``recode_store(mask=)`` take it.

    The threshold is the WHOLE volume's: ``threshold`` (a number in counts) if given; else
    ``measure.foreground_cut(k)`` of a ``StoreMeasure`` of ``src``; else the function measures ``src`` itself first
    (``measure_store``, one more pass: ``stats["passes"]`` is then 2, otherwise 1).  Seeds are the voxels above it
    (``raw >= cut`` with ``cut = floor(threshold) + 1``, clamped to 0..65536), dilated ``dilate`` (0..8) times.

    ``min_voxels`` (0..``MAX_MIN_VOXELS``; 0 and 1 filter nothing): only seeds whose connected component among the
    seeds of the WHOLE volume (``connectivity`` 6 or 26) has at least ``min_voxels`` voxels are dilated -- threshold,
    filter, dilate, as ``make_foreground_mask(..., min_voxels=, connectivity=)`` does.  A brick is then read with a
    halo of ``dilate + min_voxels - 1`` voxels, which decides every seed exactly (module docstring).

    ``src``: a path or a ``StoredArray`` opened for the device used here.  The destination is made with
    ``create_zarr`` (``chunks``: default the source's; ``codec``: default ``ExacCodec(2)``; ``attributes``).  Bricks
    are boxes of whole destination chunks (``plan_foreground``, at most ``budget_bytes`` of device memory each; a
    single chunk is taken whatever it costs).  Per brick: one region read of the brick and its halo of ``dilate``
    voxels that stays on the device, one kernel launch into a dense brick, a scatter into the pool of destination
    chunks, which is coded and committed.

    Returns ``{"threshold", "cut", "n", "n_seed", "n_kept", "n_dropped_components", "n_fg", "fraction", "cratio"}``:
    the voxels, those above the threshold (before the filter), the seeds the filter kept and the components it
    dropped, the voxels of the mask, ``n_fg / n`` and raw bytes / stored bytes.  ``stats`` (a dict) receives ``seconds``
    per phase (measure, read, mask, scatter, encode, files_write; the stream is synchronised around the phases only
    when ``stats`` is given), ``bricks``, ``passes``, ``voxels_read`` (with the halos; the measuring pass counts its
    own) and ``largest_alloc``, the most device bytes held here at one time."""
    from aind_exaspim_image_compression.utils import chunk_store, noise, store_windows, store_write
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    # -- every argument check, before a context exists
    dilate, value = _check_mask_args("foreground_store", k, dilate, threshold, value)
    min_voxels = _check_filter_args("foreground_store", min_voxels, connectivity, MAX_MIN_VOXELS)
    budget = int(budget_bytes)
    if budget < 1:
        raise ValueError("foreground_store: budget_bytes must be positive")
    chunks = store_windows.check_chunks(chunks)
    if measure is not None and not isinstance(measure, StoreMeasure):
        raise ValueError("foreground_store: measure is a StoreMeasure (utils.noise.measure_store)")
    index = int(device) if device is not None else _native.default_device()
    (arr,) = store_windows.open_u16_stores("foreground_store", (("src", src),), index)
    shape = tuple(int(s) for s in arr.shape[2:])
    if measure is not None and threshold is None and tuple(measure.shape) != shape:
        raise ValueError("foreground_store: measure was made of another shape than src")
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    codec = codec or ExacCodec(2)
    bricks = plan_foreground(shape, chunks[2:], dilate, budget, min_voxels)

    passes, voxels_read, most, measuring = 1, 0, 0, 0.0
    if threshold is not None:
        thr = float(threshold)
    else:
        if measure is None:
            t0 = time.perf_counter()
            inner = {}
            measure = noise.measure_store(arr, budget_bytes=budget, device=index, stats=inner)
            measuring = time.perf_counter() - t0
            passes, voxels_read, most = 2, inner["voxels_read"], inner["largest_alloc"]
        thr = float(measure.foreground_threshold(k))
    cut = cut_of_threshold(thr)

    ctx = _native.context(index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    source = store_windows.StoreWindows([arr], int(arr.chunks[2]))
    clock = store_windows.PhaseClock(("measure", "read", "mask", "scatter", "encode", "files_write"), stats is not None,
                                     ctx.sync)
    seconds = clock.seconds
    seconds["measure"] = measuring
    d_counts = d_kept = None
    try:
        d_counts = ctx.alloc(16)
        if min_voxels:
            d_kept = ctx.alloc(24)
        with store_windows.BrickSink("foreground_store", out, ctx, shape, chunks) as sink, \
                store_windows.capped_pools([arr], budget):
            for n_brick, brick in enumerate(bricks):
                nvox = int(np.prod(brick.extent))
                group = sink.pool([brick.origin], [brick.extent])
                t0 = time.perf_counter()
                wins, dims = source.read(brick.win_origin, brick.win_extent)
                d_brick = d_seeds = None
                try:
                    t1 = clock()
                    try:
                        if min_voxels:
                            # the kept seeds of the brick and its dilation halo; the mask kernel takes them as its window
                            s0, sd = _grown(shape, brick.origin, brick.extent, dilate)
                            scratch_bytes = _native.components_scratch_bytes(
                                _native.components_region(shape, s0, sd, min_voxels)[1], connectivity)
                            d_seeds = ctx.alloc(2 * int(np.prod(sd)))
                            most = max(most, 2 * int(np.prod(dims)) + scratch_bytes + 2 * int(np.prod(sd)) + 40)
                            with ctx.alloc(scratch_bytes) as d_scratch:
                                ctx.component_seeds_u16(wins[0], shape, brick.win_origin, dims, s0, sd, cut, min_voxels,
                                                        connectivity, count_origin=brick.origin,
                                                        count_dims=brick.extent, seeds_u16=d_seeds,
                                                        scratch=d_scratch, counts=d_kept, zero_first=n_brick == 0)
                            source.release(wins)
                            wins = []
                            d_brick = ctx.alloc(2 * nvox)
                            most = max(most, 2 * int(np.prod(sd)) + 2 * nvox + 40)
                            ctx.foreground_box_u16(d_seeds, shape, s0, sd, brick.origin, brick.extent, 1, dilate,
                                                   value, out_u16=d_brick, counts=d_counts, zero_first=n_brick == 0)
                        else:
                            d_brick = ctx.alloc(2 * nvox)
                            most = max(most, 2 * int(np.prod(dims)) + 2 * nvox + 16)
                            ctx.foreground_box_u16(wins[0], shape, brick.win_origin, dims, brick.origin, brick.extent,
                                                   cut, dilate, value, out_u16=d_brick, counts=d_counts,
                                                   zero_first=n_brick == 0)
                        t2 = clock()
                    finally:
                        source.release(wins)             # (freeing a buffer waits for the stream)
                        if d_seeds is not None:
                            d_seeds.free()
                    voxels_read += brick.window_voxels
                    with group as pool:
                        most = max(most, 2 * nvox + 2 * pool.g.pool_elems + 16)
                        pool.scatter(d_brick, nvox, np.uint16, store_write.box_records([brick.origin], brick.extent))
                        t3 = clock()
                        d_brick.free()
                        seconds["read"] += t1 - t0
                        seconds["mask"] += t2 - t1
                        seconds["scatter"] += t3 - t2
                        pool.commit()
                finally:
                    if d_brick is not None:
                        d_brick.free()
        n_seed, n_fg = (int(c) for c in d_counts.download((2,), np.uint64))
        n_kept, n_dropped = n_seed, 0
        if min_voxels:                                   # (the mask kernel counted the kept seeds as its seeds)
            n_seed, n_kept, n_dropped = (int(c) for c in d_kept.download((3,), np.uint64))
    finally:
        for buf in (d_counts, d_kept):
            if buf is not None:
                buf.free()
    n = shape[0] * shape[1] * shape[2]
    if stats is not None:
        stats.update(sink.finish(seconds), seconds=seconds, bricks=len(bricks), passes=passes, voxels_read=voxels_read,
                     largest_alloc=most)
    return {"threshold": thr, "cut": cut, "n": n, "n_seed": n_seed, "n_kept": n_kept,
            "n_dropped_components": n_dropped, "n_fg": n_fg, "fraction": n_fg / n, "cratio": 2 * n / sink.written}


def foreground_volume(vol, k=6.0, dilate=1, threshold=None, device=None, min_voxels=0, connectivity=26):
    """``foreground_store`` for a 3-D uint16 array in memory: ``make_foreground_mask(vol, k, dilate)`` as a host
    ``bool`` array.  The array is uploaded once and masked as one brick; the threshold comes from ``threshold``
    (counts) or from the table of its counts (``measure_volume``).  ``min_voxels`` (any integer >= 0: the array is
    resident) and ``connectivity`` filter the seeds by component size before the dilation."""
    vol = np.asarray(vol)
    if vol.dtype != np.uint16 or vol.ndim != 3 or 0 in vol.shape:
        raise ValueError("foreground_volume: vol is a 3-D uint16 array without an empty axis")
    dilate, _ = _check_mask_args("foreground_volume", k, dilate, threshold)
    min_voxels = _check_filter_args("foreground_volume", min_voxels, connectivity)
    shape = tuple(int(s) for s in vol.shape)
    if min_voxels and vol.size >= 2 ** 31:
        raise ValueError("foreground_volume: min_voxels takes a volume of fewer than 2^31 voxels")
    ctx = _native.context(device)
    d_vol = d_out = d_seeds = None
    try:
        d_vol = ctx.to_device(np.ascontiguousarray(vol))
        if threshold is not None:
            cut = cut_of_threshold(float(threshold))
        else:
            hist = ctx.u16_histogram(d_vol, vol.size)
            dummy = np.zeros((1, _native.measure_noise_words()), dtype=np.uint64)
            cut = StoreMeasure.from_tables(shape, hist, dummy).foreground_cut(k)
        d_out = ctx.alloc(vol.size)
        if min_voxels:
            d_seeds = ctx.alloc(2 * vol.size)
            ctx.component_seeds_u16(d_vol, shape, (0, 0, 0), shape, (0, 0, 0), shape, cut, min_voxels, connectivity,
                                    seeds_u16=d_seeds)
            ctx.foreground_box_u16(d_seeds, shape, (0, 0, 0), shape, (0, 0, 0), shape, 1, dilate, 1, out_u8=d_out)
        else:
            ctx.foreground_box_u16(d_vol, shape, (0, 0, 0), shape, (0, 0, 0), shape, cut, dilate, 1, out_u8=d_out)
        return d_out.download(shape, np.uint8).view(np.bool_)
    finally:
        for buf in (d_vol, d_out, d_seeds):
            if buf is not None:
                buf.free()
