"""The reference's two evaluation loops on the device operators (SURVEY.md section 8 row a-J).

``evaluate_blocks`` is the per-block loop of the reference's supervised evaluator (reference
``evaluate.py:88-112``): volume transform with the block's own background offset, ``predict``,
then ``compute_cratio`` and ``ssim3D(noise, denoised, data_range=max(noise))``.

``compare_with_bm4d`` is the per-patch loop of its unsupervised evaluator (reference
``evaluate.py:172-217``): the network's ``predict_patch`` against
``np.maximum(bm4d(noise, 10), 0).astype(int)`` on the patch with ``trim`` voxels removed per
side, scored by compression ratio, SSIM, mean and maximum absolute error.  The reference calls
BM4D once per patch inside the loop; here all crops go through ONE batched device call, which
changes nothing per patch (volumes of a batch are independent: tests/test_bm4d_gpu.py).

``codec`` is any object with ``encode(ndarray) -> bytes`` (the reference passes numcodecs' Blosc,
``evaluate.py:40``); without one the byte-shuffled order-0 entropy proxy of
``utils.img_util.shuffled_entropy_cratio`` is reported under the same keys (a rate proxy, not a
Blosc byte count).

``compare_stores`` is that per-block scoring -- compression ratio, SSIM, maximum-intensity projections of the noisy and
the denoised block, plus the error statistics of ``compare_with_bm4d`` -- for two *stored* volumes of any size, brick
by brick; ``compare_volumes`` is the same for arrays in memory.

File handling, plotting and CSV output of the reference classes are out of scope.
"""
import os
import time

import numpy as np

from aind_exaspim_image_compression import bm4d as _bm4d
from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning import transforms as _transforms
from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import img_util, store_compare
from aind_exaspim_image_compression.utils.store_windows import (ArrayWindows, PhaseClock, StoreWindows, capped_pools,
                                                                open_u16_stores)
from aind_exaspim_image_compression.utils.store_compare import abs_error_percentile  # noqa: F401  (public here)


def _cratio(img, codec):
    if codec is not None:
        return img_util.compute_cratio(img, codec)
    return img_util.shuffled_entropy_cratio(np.clip(img, 0, 65535).astype(np.uint16))


def evaluate_blocks(noise_imgs, model, transform, codec=None, raw_input=True, batch_size=32):
    """``{block_id: {"cratio", "ssim", "cratio_noise"}}`` for a dict of uint16 volumes.

    Each volume may carry the reference's leading singleton axes ``(1, 1, Z, Y, X)`` or
    ``(1, Z, Y, X)`` (``img_util.read(path)[0]`` there)."""
    rows = {}
    for block_id in sorted(noise_imgs):
        noise = np.asarray(noise_imgs[block_id])
        vol = noise.reshape(noise.shape[-3:])
        tf = inference.build_volume_transform(transform, vol) if raw_input else transform
        denoised = inference.predict(vol, model, tf, batch_size=batch_size, verbose=False)
        rows[block_id] = {
            "cratio": _cratio(denoised, codec),
            "cratio_noise": _cratio(vol, codec),
            "ssim": float(img_util.ssim3D(vol, denoised, data_range=np.max(vol))),
        }
    return rows


def compare_with_bm4d(patches, model, transform, codec=None, offset=None, sigma=10.0, trim=5,
                      keep_images=False):
    """Metrics of the network against BM4D for a batch ``patches[N, Z, Y, X]`` (uint16 counts).

    Returns the reference's dict of per-patch lists: ``cratio``, ``cratio_noise``, ``cratio_gt``,
    ``ssim_noise``, ``ssim_gt``, ``l1_gt``, ``lmax_gt``.  ``offset``: the brain's background
    offset for raw-input models (reference ``evaluate.py:188-193``); None keeps ``transform``.
    ``keep_images`` adds the lists ``denoised_gt`` / ``denoised`` (the images that were scored)."""
    patches = np.asarray(patches)
    if patches.ndim == 3:
        patches = patches[None]
    if patches.ndim != 4:
        raise ValueError("compare_with_bm4d expects patches[N, Z, Y, X]")
    tf = _transforms.with_offset(transform, float(offset)) if offset is not None else transform
    crop = (slice(None),) + (slice(trim, -trim),) * 3 if trim else (slice(None),) * 4
    noise = np.ascontiguousarray(patches[crop])
    gt = np.maximum(_bm4d.bm4d(noise, sigma), 0).astype(int)          # one device call for all N
    out = {k: [] for k in ("cratio_noise", "cratio_gt", "cratio", "ssim_noise", "ssim_gt", "l1_gt",
                           "lmax_gt")}
    for i in range(patches.shape[0]):
        denoised = inference.predict_patch(patches[i], model, tf)[crop[1:]]
        out["cratio"].append(_cratio(denoised, codec))
        out["cratio_noise"].append(_cratio(noise[i], codec))
        out["cratio_gt"].append(_cratio(gt[i], codec))
        out["ssim_noise"].append(float(img_util.ssim3D(noise[i], denoised)))
        out["ssim_gt"].append(float(img_util.ssim3D(gt[i], denoised)))
        out["l1_gt"].append(img_util.compute_mae(gt[i], denoised))
        out["lmax_gt"].append(img_util.compute_lmax(gt[i], denoised))
        if keep_images:
            out.setdefault("denoised_gt", []).append(gt[i])
            out.setdefault("denoised", []).append(denoised)
    return out


# ---- scoring one volume against another brick by brick ------------------------------------------
_COMPARE_PHASES = ("read", "histogram", "mips", "minmax", "ssim", "download")


def _score(ctx, shape, bricks, source, with_mask, data_range, window_size, stats):
    """The loop of ``compare_stores`` / ``compare_volumes`` over ``bricks``; ``source.read(origin, extent)`` gives the
    windows (ref, test[, mask]) and their extent as held."""
    n = shape[0] * shape[1] * shape[2]
    tables = 2 if with_mask else 1
    words = 3 * _native.mip_plane_words(shape)
    clock = PhaseClock(_COMPARE_PHASES, stats is not None, ctx.sync)
    seconds = clock.seconds
    held = {"now": 0, "most": 0}

    def hold(nbytes):
        held["now"] += nbytes
        held["most"] = max(held["most"], held["now"])

    two_pass = data_range is None
    lows = [65535, 65535]
    ssim_sum, voxels_read = 0.0, 0
    d_hist = d_planes = None
    try:
        d_hist = ctx.alloc(8 * tables * store_compare.DIFF_BINS)
        d_planes = ctx.alloc(4 * words).zero()
        hold(8 * tables * store_compare.DIFF_BINS + 4 * words)

        def sweep(first):
            """One pass over the bricks.  The first builds the table, the planes and the minima; the SSIM needs the
            data range, so it runs in the first pass when the range is given and in a second one otherwise.  A pass
            without SSIM reads the bricks alone, without their halos."""
            nonlocal ssim_sum, voxels_read
            with_ssim = not (first and two_pass)
            c1, c2 = ((0.01 * data_range) ** 2, (0.03 * data_range) ** 2) if with_ssim else (None, None)
            for k, brick in enumerate(bricks):
                w0, wn = (brick.win_origin, brick.win_extent) if with_ssim else (brick.origin, brick.extent)
                t0 = time.perf_counter()
                wins, dims = source.read(w0, wn)
                nbytes = 2 * len(wins) * dims[0] * dims[1] * dims[2]
                hold(nbytes)
                voxels_read += wn[0] * wn[1] * wn[2]
                try:
                    t1 = clock()
                    geometry = (shape, w0, dims, brick.origin, brick.extent)
                    if first:
                        ctx.diff_histogram_u16(wins[0], wins[1], wins[2] if with_mask else None, *geometry, d_hist,
                                               zero_first=k == 0)
                        t2 = clock()
                        ctx.mip3_u16(wins[0], wins[1], *geometry, d_planes)
                        t3 = clock()
                        for i in (0, 1):
                            lows[i] = min(lows[i], int(ctx.minmax(wins[i], np.uint16, dims[0] * dims[1] * dims[2])[0]))
                        t4 = clock()
                        seconds["histogram"] += t2 - t1
                        seconds["mips"] += t3 - t2
                        seconds["minmax"] += t4 - t3
                    else:
                        t4 = t1
                    if with_ssim:
                        ssim_sum += ctx.ssim3d_box_sum(wins[0], wins[1], *geometry, window_size, c1, c2)
                        seconds["ssim"] += clock() - t4
                    seconds["read"] += t1 - t0
                finally:
                    source.release(wins)             # (freeing a buffer waits for the stream)
                    hold(-nbytes)

        sweep(True)
        t0 = time.perf_counter()
        hist = d_hist.download((tables, store_compare.DIFF_BINS), np.uint64)
        planes = d_planes.download((words,), np.uint32)
        seconds["download"] += time.perf_counter() - t0
        mips = _native.split_mip_planes(planes, shape)
        highs = [int(mips[name][0].max()) for name in ("ref", "test")]
        if two_pass:
            # ssim3D's default (reference utils/img_util.py:985-988), in its arithmetic
            data_range = max(float(highs[0]) - float(lows[0]), float(highs[1]) - float(lows[1]))
            sweep(False)
    finally:
        for buf in (d_hist, d_planes):
            if buf is not None:
                buf.free()

    total = hist.sum(axis=0, dtype=np.uint64)
    out = {"n": n, "error_hist": total}
    whole = store_compare.error_stats(total, data_range)
    assert whole["n"] == n, "the bricks do not partition the volume"
    out.update({k: whole[k] for k in ("mae", "mse", "bias", "lmax", "psnr")})
    if with_mask:
        fg, bg = store_compare.error_stats(hist[0]), store_compare.error_stats(hist[1])
        out.update(error_hist_fg=hist[0], error_hist_bg=hist[1], n_fg=fg["n"], mae_fg=fg["mae"], mae_bg=bg["mae"],
                   lmax_fg=fg["lmax"], lmax_bg=bg["lmax"])
    out.update(ssim=float(np.float64(ssim_sum) / n), data_range=float(data_range),
               min={"ref": lows[0], "test": lows[1]}, max={"ref": highs[0], "test": highs[1]}, mips=mips)
    if stats is not None:
        stats.update(seconds=seconds, bricks=len(bricks), voxels_read=voxels_read, largest_alloc=held["most"],
                     passes=2 if two_pass else 1)
    return out


def _check_compare_args(window_size, data_range, budget_bytes):
    window_size, budget = int(window_size), int(budget_bytes)
    if not 1 <= window_size <= 32:
        raise ValueError("the ssim window must be 1..32")
    if budget < 1:
        raise ValueError("budget_bytes must be positive")
    if data_range is not None and not float(data_range) > 0.0:
        raise ValueError("data_range must be positive")
    return window_size, budget


def _stored_bytes(arr):
    """The bytes of a store's chunk files: what ``write_zarr`` divides the raw bytes by."""
    from aind_exaspim_image_compression.utils import chunk_store
    grid = [-(-s // c) for s, c in zip(arr.shape[2:], arr.chunks[2:])]
    return sum(os.path.getsize(os.path.join(arr.path, chunk_store.chunk_key(*idx))) for idx in np.ndindex(*grid))


def compare_stores(ref, test, mask=None, data_range=None, window_size=16, budget_bytes=4 << 30, device=None,
                   stats=None):
    """Scores the stored volume ``test`` against the stored volume ``ref`` without ever holding either: what
    ``compare_volumes(read_zarr(ref)[0, 0], read_zarr(test)[0, 0], ...)`` returns, for volumes of any size
    (DESIGN.md 5.17).

    ``ref``, ``test`` and ``mask`` (non-zero = foreground) are paths or ``StoredArray``s of uint16 and one shape,
    opened for the device used here.  Their chunk shapes may differ: bricks are boxes of whole chunks of ``ref``
    (``utils.store_compare.plan_compare``, each at most ``budget_bytes`` of device memory; a single chunk is taken
    whatever it costs), and ``test`` and ``mask`` are read by region, whatever chunks that touches.  Per brick the
    stores' windows -- the brick and the halo its SSIM reads -- come from region reads that stay on the device, and
    three kernels score the brick inside them: the signed difference table, the maximum projections and the SSIM sum
    of the box.  Nothing is carried between bricks: a halo is read again by every brick that needs it.

    ``data_range``: the ``L`` of SSIM's constants and of the PSNR.  With one given the stores are read once
    (``evaluate_blocks`` passes ``max(ref)``).  With ``None`` it is ``ssim3D``'s default, ``max(hi_ref - lo_ref,
    hi_test - lo_test)``, which is only known after all of both volumes has been seen: a first pass builds the table,
    the projections and the extremes from the bricks alone, and a second pass over the windows computes the SSIM --
    **every chunk is read and decoded twice** (the halos only in the second pass).

    Returns a dict: ``n`` (voxels); ``error_hist`` (131071 uint64 bins, ``test - ref + 65535``), and with a mask
    ``error_hist_fg`` / ``error_hist_bg``; from the table, in exact integer arithmetic and one float64 division
    each, ``mae``, ``mse``, ``bias`` (mean signed error), ``lmax`` and ``psnr`` (``10 log10(data_range^2 / mse)``,
    ``inf`` for equal stores), with a mask also ``mae_fg``, ``mae_bg``, ``lmax_fg``, ``lmax_bg``, ``n_fg``
    (``abs_error_percentile`` gives any percentile of the error from the table); ``ssim`` and ``data_range``; ``min``
    and ``max`` (``{"ref", "test"}``); ``cratio_ref`` / ``cratio_test`` (raw bytes over chunk-file bytes, what
    ``write_zarr`` returned); and ``mips``: ``{"ref" | "test" | "abs_diff": (yx, zx, zy)}``, host uint16 planes
    (``img_util.mip_to_uint8`` stretches one for viewing).  Everything but ``ssim`` is independent of the brick plan;
    ``ssim`` changes with it only by the order of the final fp64 sum.

    ``stats`` (a dict) receives ``seconds`` per phase (read, histogram, mips, minmax, ssim, download; the stream is
    synchronised around the phases only when ``stats`` is given), ``bricks``, ``passes``, ``voxels_read`` -- per store,
    halos included, so ``voxels_read / n`` shows the share read more than once -- and ``largest_alloc``, the most
    device bytes held here at one time (the readers' pools of decoded chunks are theirs and are not counted)."""
    window_size, budget = _check_compare_args(window_size, data_range, budget_bytes)
    index = int(device) if device is not None else _native.default_device()
    arrs = open_u16_stores("compare_stores", (("ref", ref), ("test", test), ("mask", mask)), index)
    shape = tuple(int(s) for s in arrs[0].shape[2:])
    chunks = tuple(int(c) for c in arrs[0].chunks[2:])
    with_mask = mask is not None
    bricks = store_compare.plan_compare(shape, chunks, window_size, budget, with_mask)
    ctx = _native.context(index)
    with capped_pools(arrs, budget):
        out = _score(ctx, shape, bricks, StoreWindows(arrs, chunks[0]), with_mask, data_range, window_size, stats)
    raw = 2 * shape[0] * shape[1] * shape[2]
    out.update(cratio_ref=raw / _stored_bytes(arrs[0]), cratio_test=raw / _stored_bytes(arrs[1]))
    return out


def compare_volumes(ref, test, mask=None, data_range=None, window_size=16, device=None, stats=None):
    """``compare_stores`` for uint16 arrays in memory: the volumes are uploaded whole and scored as one brick.  The
    same dict without the compression ratios; ``mask``: any array of the volumes' shape, non-zero = foreground."""
    window_size, _ = _check_compare_args(window_size, data_range, 1)
    arrays = [np.asarray(ref), np.asarray(test)]
    for a in arrays:
        if a.dtype != np.uint16 or a.ndim != 3:
            raise ValueError("compare_volumes: ref and test are 3-D uint16 arrays")
    if mask is not None:
        arrays.append((np.asarray(mask) != 0).astype(np.uint16))
    if any(a.shape != arrays[0].shape for a in arrays) or 0 in arrays[0].shape:
        raise ValueError("compare_volumes: ref, test and mask must have one shape, without an empty axis")
    shape = tuple(int(s) for s in arrays[0].shape)
    ctx = _native.context(device)
    brick = store_compare.Brick((0, 0, 0), shape, (0, 0, 0), shape, 2 * len(arrays) * int(np.prod(shape)))
    source = ArrayWindows(ctx, [np.ascontiguousarray(a) for a in arrays])
    try:
        return _score(ctx, shape, [brick], source, mask is not None, data_range, window_size, stats)
    finally:
        source.close()
