"""Re-coding a store under a mask store, out of core: ``recode_store`` is
``write_zarr(read_zarr(src)[0, 0], dst_path, chunks, codec, mask=read_zarr(mask)[0, 0])`` for a volume of any size --
the block-bounded codec's "foreground within fg_max_error, background within max_error" with the mask that
``foreground_store`` makes."""
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_compare
from aind_exaspim_image_compression.utils.store_predict import POOL_BYTES

MASK_BYTES = 2              # per voxel of the brick: the mask window as bytes, and the mask pool


def _brick_window(b0, bd, dim):
    return b0, bd


def plan_recode(shape, chunks_zyx, budget_bytes, with_mask=False):
    """The bricks (``store_compare.Brick``) of re-coding a volume of ``shape`` into chunks of ``chunks_zyx``: boxes of
    whole destination chunks that partition the volume (``store_compare.plan_bricks``); a brick's window is the brick.
    A brick costs its windows (the source's, and the mask's ``with_mask``) at 2 bytes a voxel as they are held, each
    reader's pool of decoded chunks, and per voxel the destination pool with its coded streams (and the two byte
    masks)."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    budget = int(budget_bytes)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_recode: shape and chunks are three positive sizes each")
    if budget < 1:
        raise ValueError("plan_recode: budget_bytes >= 1")
    return store_compare.plan_bricks(shape, chunk, budget, 2 if with_mask else 1, _brick_window,
                                     POOL_BYTES + (MASK_BYTES if with_mask else 0))


def recode_store(src, dst_path, codec=None, mask=None, chunks=None, attributes=None, budget_bytes=4 << 30, device=None,
                 stats=None):
    """The stored uint16 volume ``src`` coded anew -- another codec, other chunks, or a block-bounded codec under the
    mask store ``mask`` (uint16, non-zero = foreground: what ``foreground_store`` writes) -- without ever holding the
    volume.  ``dst_path`` is, chunk file for chunk file, ``write_zarr(read_zarr(src)[0, 0], dst_path, chunks, codec,
    mask=read_zarr(mask)[0, 0])``; returns what ``write_zarr`` returns, raw bytes / stored chunk bytes.

    ``codec``: any codec ``create_zarr`` takes (default ``ExacCodec(2)``), ``BlockBoundedCodec.from_noise`` with its
    bound table included.  ``mask`` goes only with a codec that takes one (``ValueError`` otherwise, as from
    ``write_zarr``) and has the source's shape.  ``chunks``: default the source's.  Bricks are boxes of whole
    destination chunks (``plan_recode``, at most ``budget_bytes`` of device memory each).  Per brick: one region read
    of the source (and of the mask) that stays on the device, the counts scattered into the pool of destination
    chunks, the mask turned into bytes (``exabm4d_nonzero_u8_dev``) and scattered into the mask pool; the pool is
    coded and committed.  ``stats`` (a dict) receives ``seconds`` per phase (read, scatter, encode, files_write),
    ``bricks``, ``voxels_read`` per store and ``largest_alloc``."""
    from aind_exaspim_image_compression.utils import chunk_store, store_windows, store_write
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    # -- every argument check, before a context exists
    codec = codec or ExacCodec(2)
    if mask is not None and not codec.takes_mask:
        raise ValueError("only a BlockBoundedCodec takes a mask")
    budget = int(budget_bytes)
    if budget < 1:
        raise ValueError("recode_store: budget_bytes must be positive")
    chunks = store_windows.check_chunks(chunks)
    index = int(device) if device is not None else _native.default_device()
    arrs = store_windows.open_u16_stores("recode_store", (("src", src), ("mask", mask)), index)
    shape = tuple(int(s) for s in arrs[0].shape[2:])
    chunks = chunks if chunks is not None else tuple(int(c) for c in arrs[0].chunks)
    with_mask = mask is not None
    bricks = plan_recode(shape, chunks[2:], budget, with_mask)

    ctx = _native.context(index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    source = store_windows.StoreWindows(arrs, int(arrs[0].chunks[2]))
    clock = store_windows.PhaseClock(("read", "scatter", "encode", "files_write"), stats is not None, ctx.sync)
    seconds = clock.seconds
    voxels_read, most = 0, 0
    with store_windows.BrickSink("recode_store", out, ctx, shape, chunks) as sink, \
            store_windows.capped_pools(arrs, budget):
        for brick in bricks:
            group = sink.pool([brick.origin], [brick.extent], want_mask=with_mask)
            t0 = time.perf_counter()
            wins, dims = source.read(brick.win_origin, brick.win_extent)
            voxels_read += brick.window_voxels
            n_win = int(np.prod(dims))
            held = list(wins)                            # and the mask as bytes
            try:
                t1 = clock()
                with group as pool:
                    # the window may be taller than the brick (whole z slabs): its first brick.extent layers count
                    record = store_write.box_records([brick.origin], brick.extent)
                    record["stride_z"], record["stride_y"] = dims[1] * dims[2], dims[2]
                    pool.scatter(wins[0], n_win, np.uint16, record)
                    if with_mask:
                        d_bytes = ctx.alloc(n_win)
                        held.append(d_bytes)
                        ctx.nonzero_u8(wins[1], n_win, d_bytes)
                        pool.scatter(d_bytes, n_win, np.uint8, record, mask=True)
                    most = max(most, (2 * len(wins) + (1 if with_mask else 0)) * n_win +
                               (3 if with_mask else 2) * pool.g.pool_elems)
                    t2 = clock()
                    source.release(held)                 # before the pool is coded (freeing waits for the stream)
                    seconds["read"] += t1 - t0
                    seconds["scatter"] += t2 - t1
                    pool.commit()
            finally:
                source.release(held)
    if stats is not None:
        stats.update(sink.finish(seconds), seconds=seconds, bricks=len(bricks), voxels_read=voxels_read,
                     largest_alloc=most)
    return 2 * shape[0] * shape[1] * shape[2] / sink.written
