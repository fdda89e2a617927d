"""What the loops that walk a store brick by brick share (``evaluate.compare_stores``, DESIGN.md 5.17;
``utils.noise.measure_store``, 5.18; the store-to-store operators, 5.14, 5.16, 5.19 - 5.23).  The read side: the stores
of one call opened and checked, and one region read per store and brick that stays on the device.  The write side: the
checks of a destination's arguments, a clock of the phases, and ``BrickSink``, which takes bricks of whole destination
chunks from device buffers, codes them and commits their chunk files."""
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_write
from aind_exaspim_image_compression.utils.store_predict import READER_SHARE, window_slabs


def check_chunks(chunks):
    """``chunks`` as five ints, None for None; ``ValueError`` for anything but ``(1, 1, cz, cy, cx)``."""
    if chunks is None:
        return None
    try:
        chunks = tuple(int(c) for c in chunks)
    except TypeError:
        raise ValueError("chunks must be (1, 1, cz, cy, cx)") from None
    if len(chunks) != 5 or chunks[:2] != (1, 1) or min(chunks) < 1:
        raise ValueError("chunks must be (1, 1, cz, cy, cx)")
    return chunks


def check_store_args(who, chunks, codec, budget_bytes):
    """``(chunks, codec, budget)`` of a destination's arguments, checked: ``codec`` defaults to ``ExacCodec(2)``."""
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    budget = int(budget_bytes)
    if budget < 1:
        raise ValueError("%s: budget_bytes must be positive" % who)
    chunks = check_chunks(chunks)
    codec = codec or ExacCodec(2)
    if not hasattr(codec, "config_entry") or getattr(codec, "typesize", None) != 2:
        raise ValueError("%s: codec must be a codec of uint16 volumes that create_zarr takes" % who)
    return chunks, codec, budget


class PhaseClock:
    """The seconds per phase of a loop: ``seconds`` holds a sum per name of ``phases``, and calling the clock gives the
    time -- after ``sync()``, so that a phase ends with its kernels, when ``timed``; as it is otherwise."""

    def __init__(self, phases, timed, sync):
        self.seconds = dict.fromkeys(phases, 0.0)
        self.timed, self.sync = timed, sync

    def __call__(self):
        if self.timed:
            self.sync()
        return time.perf_counter()


def open_u16_stores(who, named, index):
    """The ``StoredArray``s of ``named`` -- ``(name, path or StoredArray or None)`` pairs, None left out -- after the
    checks such a loop needs before any context exists: uint16, one shape, opened for device ``index``."""
    from aind_exaspim_image_compression.utils import chunk_store
    arrs = []
    for name, src in named:
        if src is None:
            continue
        try:
            arr = src if hasattr(src, "read_patches") else chunk_store.open_zarr(src, device=index)
        except NotImplementedError as e:
            raise ValueError("%s: %s must hold uint16 (%s)" % (who, name, e)) from None
        if np.dtype(arr.dtype) != np.uint16:
            raise ValueError("%s: %s must hold uint16" % (who, name))
        if int(arr.device if arr.device is not None else _native.default_device()) != index:
            raise ValueError("%s: %s was opened for another device than %d, the one used here" % (who, name, index))
        if arrs and tuple(arr.shape) != tuple(arrs[0].shape):
            raise ValueError("%s: %s must have one shape" % (who, ", ".join(n for n, _ in named)))
        arrs.append(arr)
    return arrs


class capped_pools:
    """While the block runs, every reader's pool of decoded chunks is capped at ``budget // READER_SHARE``."""

    def __init__(self, arrs, budget):
        self.arrs, self.budget = arrs, budget

    def __enter__(self):
        self.caps = [a.max_pool_bytes for a in self.arrs]
        for a in self.arrs:
            a.max_pool_bytes = max(1, min(a.max_pool_bytes, self.budget // READER_SHARE))

    def __exit__(self, *exc):
        for a, cap in zip(self.arrs, self.caps):
            a.max_pool_bytes = cap


class StoreWindows:
    """Windows of one to three stores: one region read per store and brick, in z slabs of about a chunk of the first
    store so that each reader's pool of decoded chunks stays under its cap; the slabs lie one after another in one
    allocation, and layers past the volume's last hold ``fill``: 65535 (never the minimum, never scored) unless the
    caller says otherwise."""

    def __init__(self, arrs, chunk_z, fill=65535):
        self.arrs, self.chunk_z, self.fill = arrs, chunk_z, fill

    def read(self, origin, extent):
        slabs, slab = window_slabs(extent[0], self.chunk_z)
        starts = [(origin[0] + j * slab, origin[1], origin[2]) for j in range(slabs)]
        wins = []
        try:
            for arr in self.arrs:
                wins.append(arr.read_patches(starts, (slab, extent[1], extent[2]), is_center=False, out="device",
                                             fill=self.fill))
        except BaseException:
            self.release(wins)
            raise
        return wins, (slabs * slab, extent[1], extent[2])

    @staticmethod
    def release(wins):
        for w in wins:
            w.free()

    def close(self):
        pass


class ArrayWindows:
    """Arrays in memory as their own windows: uploaded once, one brick."""

    def __init__(self, ctx, arrays):
        self.shape = arrays[0].shape
        self.bufs = []
        try:
            for a in arrays:
                self.bufs.append(ctx.to_device(a))
        except BaseException:
            self.close()
            raise

    def read(self, origin, extent):
        return self.bufs, self.shape

    @staticmethod
    def release(wins):
        pass

    def close(self):
        for b in self.bufs:
            b.free()


class BrickSink:
    """The write side of a store-to-store loop: bricks of whole chunks of the new store ``out`` (``create_zarr``; of
    ``shape`` in ``chunks``), taken from device buffers, coded and committed.  A context manager: it holds the write
    codec's bound table on the device while the block runs.  ``st`` are the write's counts (``store_write``),
    ``written`` the bytes of the chunk files so far; ``box`` names a box in the error message."""

    def __init__(self, who, out, ctx, shape, chunks, box="brick"):
        self.who, self.out, self.ctx, self.shape, self.chunk3, self.box = who, out, ctx, shape, chunks[2:], box
        self.st, self.written, self.d_table = store_write._new_stats(), 0, None

    def __enter__(self):
        self.d_table = store_write.bound_table_on_device(self.out, self.ctx)
        return self

    def __exit__(self, *exc):
        if self.d_table is not None:
            self.d_table.free()

    def pool(self, origins, extents, want_mask=False):
        """The pool of the chunks that the boxes at ``origins`` of ``extents`` cover, planned here -- ``RuntimeError``
        unless one box alone covers each chunk, so that none is read back -- and a context manager: the pool is
        allocated on entry and freed on exit, so a loop may plan before it reads and open after its kernel."""
        return _SinkPool(self, origins, extents, want_mask)

    def finish(self, seconds):
        """After the last brick: the encode and files_write seconds into ``seconds``; returns the ``stats`` entries
        every operator reports."""
        seconds["encode"], seconds["files_write"] = self.st["seconds"]["encode"], self.st["seconds"]["files_write"]
        return {"chunks": self.st["chunks"], "encode_calls": self.st["encode_calls"]}


class _SinkPool:
    """One group of a ``BrickSink``: ``g`` its ``store_write.WriteGroup``."""

    def __init__(self, sink, origins, extents, want_mask):
        self.sink, self.want_mask, self.pool = sink, want_mask, None
        (self.g,) = store_write.plan_write(sink.shape, sink.chunk3, origins, extents, sink.out._nominal,
                                           exists=lambda *idx: False, max_pool_bytes=1 << 62)
        if any(s != store_write.COVERED for s in self.g.states):
            raise RuntimeError("%s: a destination chunk is not covered by one %s" % (sink.who, sink.box))

    def __enter__(self):
        self.pool = store_write.open_pool(self.sink.out, self.sink.ctx, self.g, self.sink.st, want_mask=self.want_mask)
        return self

    def __exit__(self, *exc):
        self.pool.free()

    def scatter(self, src, n_elems, dtype, records, mask=False, dst_boxes=None):
        """Boxes of the device buffer ``src`` (``records``: their ``BOX_SRC`` records) into the pool, or with ``mask``
        bytes into the mask pool.  ``dst_boxes``: as ``store_write.scatter`` takes it.  Asynchronous."""
        store_write.scatter(self.sink.ctx, self.g, self.pool, src, n_elems, dtype, records, dst_boxes=dst_boxes,
                            mask=mask)

    def commit(self):
        """The pool coded and its chunk files replaced (``store_write.encode_commit``)."""
        sink = self.sink
        sink.written += store_write.encode_commit(sink.out, sink.ctx, self.g, self.pool, sink.st, sink.d_table)
