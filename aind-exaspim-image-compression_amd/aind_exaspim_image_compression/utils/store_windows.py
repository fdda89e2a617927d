"""Windows of stored volumes on the device, for the loops that walk a store brick by brick (``evaluate.compare_stores``,
DESIGN.md 5.17; ``utils.noise.measure_store``, 5.18): the stores of one call opened and checked, and one region read
per store and brick that stays on the device."""
import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils.store_predict import READER_SHARE, window_slabs


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
    allocation, and layers past the volume's last hold 65535 (never the minimum, never scored)."""

    def __init__(self, arrs, chunk_z):
        self.arrs, self.chunk_z = arrs, chunk_z

    def read(self, origin, extent):
        slabs, slab = window_slabs(extent[0], self.chunk_z)
        starts = [(origin[0] + j * slab, origin[1], origin[2]) for j in range(slabs)]
        wins = []
        try:
            for arr in self.arrs:
                wins.append(arr.read_patches(starts, (slab, extent[1], extent[2]), is_center=False, out="device",
                                             fill=65535))
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
