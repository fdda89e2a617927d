"""Label stores read by regions: boxes and patch batches straight from the coded chunks.

The reference reads 64^3 label patches out of its ``tensorstore`` segmentation in ``sample_segmentation_voxel``,
``annotation_mask`` and the coherence gate of ``sample_clean`` (reference ``machine_learning/data_handling.py``).
``LabelArray`` (``chunk_store.open_zarr`` of an ``exac-labels`` store) answers those reads:

* ``plan_label_read`` (host, numpy) finds the chunks N boxes of one shape touch and puts the boxes into consecutive
  groups whose **coded** chunks fit ``max_pool_bytes``;
* per group the touched chunk files are read once each, every stream's header and block table is validated on the
  host (``label_codec.validate_stream``: a corrupt file raises ``ValueError`` before any device call), the streams are
  packed into one container, uploaded, and one ``exabm4d_label_gather_boxes_dev`` call (``csrc/
  label_codec_kernels.hip``) unpacks exactly the block rows the boxes intersect.  There is no decoded pool.

Writes take whole chunks only (``__setitem__`` of a box aligned to the chunk grid or the array's edge): enough to
build a whole-brain label store slab by slab, byte for byte what ``write_zarr`` makes of the whole array.
"""
import json
import os
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.label_codec import LabelCodec, validate_stream
from aind_exaspim_image_compression.utils.store_read import DevicePatches, normalize_key


class LabelGroup:
    """Boxes ``[first, stop)`` of a plan and what they need: ``chunks`` (M, 3) touched chunk indices in raster order,
    ``box_srcs`` (stop - first, per_box) int32 -- per box the rows of ``chunks`` of its chunk range, in raster order
    over that range (-1 = unused) -- and ``coded_bytes``, the sum of those chunks' stream lengths."""

    def __init__(self, first, stop, chunks, box_srcs, coded_bytes):
        self.first, self.stop, self.chunks, self.box_srcs, self.coded_bytes = first, stop, chunks, box_srcs, coded_bytes


def plan_label_read(shape3, chunk3, starts, box, coded_bytes, max_pool_bytes=1 << 30):
    """The plan of reading N boxes of shape ``box`` at ``starts`` (N, 3; any integers, inside the array or not) from a
    label array of ``shape3`` in chunks of ``chunk3``: a list of ``LabelGroup``.  ``coded_bytes((iz, iy, ix))`` is the
    stream length of a chunk (the store passes its file sizes).  Boxes go into consecutive groups whose coded chunks
    (deduplicated within the group, each padded to 16 bytes) and table rows (12 + 4 per touched chunk bytes a box, 40 a
    chunk) fit ``max_pool_bytes``; a group holds at least one box.  A box wholly outside the array touches nothing."""
    shape = tuple(int(s) for s in shape3)
    chunk = tuple(int(c) for c in chunk3)
    box = tuple(int(b) for b in box)
    if len(shape) != 3 or len(chunk) != 3 or len(box) != 3 or min(shape) < 1 or min(chunk) < 1 or min(box) < 1:
        raise ValueError("plan_label_read: shape, chunk and box are three positive sizes each")
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
    lo = np.maximum(starts, 0) // np.array(chunk)
    hi = (np.minimum(starts + np.array(box), np.array(shape)) - 1) // np.array(chunk)
    inside = np.all((starts < np.array(shape)) & (starts + np.array(box) > 0), axis=1)

    def ids_of(n):
        if not inside[n]:
            return []
        z, y, x = (np.arange(lo[n, a], hi[n, a] + 1) for a in range(3))
        return ((z[:, None, None] * grid[1] + y[None, :, None]) * grid[2] + x[None, None, :]).reshape(-1).tolist()

    def index_of(i):
        return (i // (grid[1] * grid[2]), i // grid[2] % grid[1], i % grid[2])

    sizes = {}

    def nbytes(i):
        if i not in sizes:
            sizes[i] = 40 + -(-int(coded_bytes(index_of(i))) // 16) * 16
        return sizes[i]

    def build(first, stop, held, box_ids):
        ids = sorted(held)
        row_of = {i: m for m, i in enumerate(ids)}
        per_box = max([len(b) for b in box_ids] + [1])
        box_srcs = np.full((stop - first, per_box), -1, dtype=np.int32)
        for n, b in enumerate(box_ids):
            box_srcs[n, :len(b)] = [row_of[i] for i in b]
        chunks = np.array([index_of(i) for i in ids], dtype=np.int64).reshape(-1, 3)
        return LabelGroup(first, stop, chunks, box_srcs, sum(nbytes(i) - 40 for i in ids))

    groups, first, held, held_bytes, box_ids = [], 0, set(), 0, []
    for n in range(len(starts)):
        ids = ids_of(n)
        own = 12 + 4 * len(ids)
        more = own + sum(nbytes(i) for i in ids if i not in held)
        if n > first and held_bytes + more > max_pool_bytes:
            groups.append(build(first, n, held, box_ids))
            first, held, held_bytes, box_ids = n, set(), 0, []
            more = own + sum(nbytes(i) for i in ids)
        held.update(ids)
        held_bytes += more
        box_ids.append(ids)
    if len(starts):
        groups.append(build(first, len(starts), held, box_ids))
    return groups


class LabelArray:
    """A stored (1, 1, z, y, x) uint32 / uint64 label volume (``exac-labels``) read by regions
    (``chunk_store.open_zarr``) and, opened with ``mode="r+"`` (or made by ``chunk_store.create_zarr``), written by
    whole chunks."""

    ndim = 5

    def __init__(self, path, device=None, max_pool_bytes=1 << 30, mode="r", codec=None):
        if mode not in ("r", "r+"):
            raise ValueError("LabelArray: mode is 'r' or 'r+'")
        with open(os.path.join(path, "zarr.json")) as f:
            self.meta = json.load(f)
        shape3, chunk3, typesize, _ = chunk_store.check_metadata(self.meta)
        entry = self.meta["codecs"][0]
        if entry["name"] != LabelCodec.codec_id:
            raise ValueError("LabelArray: not an exac-labels store")
        if codec is not None and (not isinstance(codec, LabelCodec) or
                                  codec.config_entry() != entry["configuration"]):
            raise ValueError("open_zarr: the codec passed is not the one the store was written with")
        self.path = path
        self.shape = (1, 1) + shape3
        self.chunks = (1, 1) + chunk3
        self.device = device
        self.max_pool_bytes = int(max_pool_bytes)
        self.mode = mode
        self._codec = LabelCodec(typesize, device=device)
        self.dtype = self._codec.dtype
        self.last_read = None
        self.last_write = None

    def __len__(self):
        return 1

    def _chunk_path(self, idx):
        return os.path.join(self.path, chunk_store.chunk_key(*idx))

    def _extent(self, idx):
        return tuple(min(c, s - int(i) * c) for i, c, s in zip(idx, self.chunks[2:], self.shape[2:]))

    # -- reads -----------------------------------------------------------------------------------
    def __getitem__(self, key):
        starts, stops, shape = normalize_key(key, self.shape)
        if 0 in shape or any(b <= a for a, b in zip(starts, stops)):
            return np.empty(shape, dtype=self.dtype)
        box = tuple(b - a for a, b in zip(starts[2:], stops[2:]))
        return self.read_patches([starts[2:]], box, is_center=False)[0].reshape(shape)

    def read_patches(self, voxels, patch_shape, is_center=True, out="host"):
        """(N, *patch_shape) label patches at ``voxels`` (N, 3), placed as ``StoredArray.read_patches`` places them
        (box n starts at ``voxel - d // 2`` per axis, or at ``voxel`` with ``is_center=False``); voxels outside the
        array are 0.  ``out="device"`` returns a ``DevicePatches``.  ``max_pool_bytes`` bounds the coded chunks held
        on the device at a time, not the output, which is one device allocation of the whole batch.  Every chunk
        file of a group is validated before anything of the group is uploaded; a missing file raises
        ``FileNotFoundError``.  ``last_read`` describes the last call that succeeded in full."""
        if out not in ("host", "device"):
            raise ValueError("read_patches: out is 'host' or 'device'")
        box = tuple(int(d) for d in patch_shape)
        if len(box) != 3 or min(box) < 1:
            raise ValueError("read_patches: patch_shape is three positive sizes")
        starts = np.asarray(voxels)
        if starts.size and not np.issubdtype(starts.dtype, np.integer):
            if not (np.issubdtype(starts.dtype, np.floating) and np.all(starts == np.rint(starts))):
                raise ValueError("read_patches: voxels are integer coordinates")
        starts = starts.astype(np.int64).reshape(-1, 3)
        if is_center:
            starts = starts - np.array([d // 2 for d in box])
        if starts.size and (starts.min() < -2 ** 31 or (starts + np.array(box)).max() >= 2 ** 31):
            raise ValueError("read_patches: a box outside the int32 coordinate range")
        n, shape = len(starts), (len(starts),) + box
        self.last_read = {"chunks": 0, "chunk_bytes": 0, "gather_calls": 0, "groups": 0,
                          "seconds": {"files": 0.0, "validate": 0.0, "upload": 0.0, "gather": 0.0}}
        if n == 0:
            return np.empty(shape, dtype=self.dtype) if out == "host" else DevicePatches(None, shape, self.dtype)
        ctx = d_out = None
        box_bytes = box[0] * box[1] * box[2] * self.dtype.itemsize
        try:
            groups = plan_label_read(self.shape[2:], self.chunks[2:], starts, box,
                                     lambda idx: os.path.getsize(self._chunk_path(idx)), self.max_pool_bytes)
            for g in groups:
                blobs = self._load_group(g)             # read and validated: nothing has gone to the device yet
                if ctx is None:
                    ctx = _native.context(self.device)
                    d_out = ctx.alloc(n * box_bytes)
                self._gather_group(ctx, g, blobs, starts, box, int(d_out.ptr) + g.first * box_bytes)
            if out == "device":
                res, d_out = DevicePatches(d_out, shape, self.dtype), None
                return res
            return d_out.download(shape, self.dtype)
        except BaseException:
            self.last_read = None                   # a failed read is not described
            raise
        finally:
            if d_out is not None:
                d_out.free()

    def _load_group(self, g):
        t0 = time.perf_counter()
        blobs = []
        for idx in g.chunks:
            with open(self._chunk_path(idx), "rb") as f:
                blobs.append(f.read())
        t1 = time.perf_counter()
        for idx, blob in zip(g.chunks, blobs):
            try:
                validate_stream(blob, self.dtype.itemsize, self._extent(idx))
            except ValueError as e:
                raise ValueError(f"chunk {tuple(int(i) for i in idx)} of {self.path}: {e}") from None
        self.last_read["seconds"]["files"] += t1 - t0
        self.last_read["seconds"]["validate"] += time.perf_counter() - t1
        return blobs

    def _gather_group(self, ctx, g, blobs, starts, box, out_ptr):
        t0 = time.perf_counter()
        data, offsets, sizes = chunk_store.pack_streams(blobs)
        srcs = np.zeros(len(blobs), dtype=_native.LABEL_SRC)
        for m, idx in enumerate(g.chunks):
            rec = srcs[m]
            rec["offset"], rec["bytes"] = int(offsets[m]), int(sizes[m])
            rec["z0"], rec["y0"], rec["x0"] = (int(i) * c for i, c in zip(idx, self.chunks[2:]))
            rec["ez"], rec["ey"], rec["ex"] = self._extent(idx)
        d_data = ctx.to_device(data if data.size else np.zeros(16, np.uint8))
        t1 = time.perf_counter()
        try:
            ctx.label_gather_boxes(d_data, data.size, self.dtype.itemsize, srcs, g.box_srcs, starts[g.first:g.stop],
                                   box, self.shape[2:], self.chunks[2:], out_ptr)       # synchronises
        finally:
            d_data.free()
        self.last_read["seconds"]["upload"] += t1 - t0
        self.last_read["seconds"]["gather"] += time.perf_counter() - t1
        self.last_read["chunks"] += len(blobs)
        self.last_read["chunk_bytes"] += sum(len(b) for b in blobs)
        self.last_read["gather_calls"] += 1
        self.last_read["groups"] += 1

    # -- writes: whole chunks only -----------------------------------------------------------------
    def __setitem__(self, key, value):
        """``arr[0, 0, z0:z1, y0:y1, x0:x1] = value`` for a box whose every face lies on the chunk grid or on the
        array's edge (``ValueError`` otherwise, before a byte is written): ``value`` is an array of exactly the
        result shape and the store's dtype (or any unsigned integer type it holds), or a scalar.  The chunks are coded
        in one ``encode_device`` call and each file is replaced atomically, after all of them have been coded."""
        if self.mode != "r+":
            raise ValueError("LabelArray: the store was opened read-only (mode='r')")
        starts, stops, shape = normalize_key(key, self.shape)
        lo, hi = starts[2:], stops[2:]
        for a, b, c, s in zip(lo, hi, self.chunks[2:], self.shape[2:]):
            if b <= a:
                raise ValueError("LabelArray: an empty box")
            if a % c or (b % c and b != s):
                raise ValueError("LabelArray: a write covers whole chunks -- a box aligned to the chunk grid or to "
                                 "the array's edge")
        box = tuple(b - a for a, b in zip(lo, hi))
        v = np.asarray(value)
        if v.dtype.kind not in "ub" or v.dtype.itemsize > self.dtype.itemsize:
            if not (v.dtype.kind == "i" and v.size and v.min() >= 0 and int(v.max()) < 2 ** (8 * self.dtype.itemsize)):
                raise ValueError(f"LabelArray: values must be unsigned integers that {self.dtype} holds")
        if v.ndim and v.shape != shape:
            raise ValueError(f"LabelArray: the value's shape {v.shape} is not the box's {shape}")
        vol = np.ascontiguousarray(np.broadcast_to(v.astype(self.dtype), shape).reshape(box))
        t0 = time.perf_counter()
        self.last_write = None
        ctx = _native.context(self.device)
        with ctx.to_device(vol.reshape(-1)) as d_vol:
            enc = self._codec.encode_device(ctx, d_vol, box, self.chunks[2:])
        t1 = time.perf_counter()
        first = [a // c for a, c in zip(lo, self.chunks[2:])]
        grid = [-(-b // c) for b, c in zip(box, self.chunks[2:])]
        total, k = 0, 0
        for iz in range(grid[0]):
            for iy in range(grid[1]):
                for ix in range(grid[2]):
                    blob = enc.chunk_bytes(k)
                    final = self._chunk_path((first[0] + iz, first[1] + iy, first[2] + ix))
                    os.makedirs(os.path.dirname(final), exist_ok=True)
                    tmp = os.path.join(os.path.dirname(final), ".%s.%d.tmp" % (os.path.basename(final), os.getpid()))
                    try:
                        with open(tmp, "wb") as f:
                            f.write(blob)
                        os.replace(tmp, final)
                    except BaseException:
                        if os.path.exists(tmp):
                            os.remove(tmp)
                        raise
                    total += len(blob)
                    k += 1
        self.last_write = {"chunks": k, "chunk_bytes": total, "encode_calls": 1, "groups": 1,
                           "seconds": {"encode": t1 - t0, "files_write": time.perf_counter() - t1}}
