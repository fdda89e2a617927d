"""Region reads of a chunk store: boxes and patch batches that decode only the chunks they touch.

The reference touches a stored volume in one way: small boxes at arbitrary voxels -- ``self.imgs[brain_id][(0, 0,
*s)]`` in ``TrainDataset.read_patch`` (reference ``machine_learning/data_handling.py:741-758``), ``img[0, 0, z0:z1,
y0:y1, x0:x1]`` in ``get_patch`` (``utils/img_util.py:271-305``), the candidate batches of ``sample_bright_voxel`` and
the evaluators.  ``StoredArray`` (``chunk_store.open_zarr``) answers those against a store ``chunk_store.write_zarr``
wrote, in any of its three formats:

* ``plan_read`` (host, numpy) finds the chunks N boxes of one shape touch, lays them out as at most eight virtual
  volumes ("stacks") that the existing decode entries take unchanged -- a chunk stream is position-independent apart
  from its extent -- and lists, per box, where each decoded chunk lies;
* per group of boxes the touched chunk files are read once each, every stack is decoded with one
  ``decode_device`` call into one pool allocation, and one ``exabm4d_gather_boxes_dev`` call (``csrc/
  region_kernels.hip``) cuts all boxes out of the pool, as uint16 or as ``float32 - offset`` (``read_counts``).
"""
import json
import operator
import os
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume

POOL_ALIGN = 128        # elements: every stack starts on a 256-byte boundary of the pool


class Stack:
    """Chunks of one extent class as one virtual volume: ``members`` (rows of the group's ``chunks``) are its chunks
    0, 1, ... along ``axis``; it decodes as a volume of ``shape`` with chunk shape ``chunk`` to pool element
    ``base``."""

    def __init__(self, shape, chunk, axis, members, base):
        self.shape, self.chunk, self.axis, self.members, self.base = shape, chunk, axis, members, base


class Group:
    """Boxes ``[first, stop)`` of a plan and what they need: ``chunks`` (M, 3) touched chunk indices in raster
    order, ``stacks``, ``srcs`` (M ``_native.BOX_SRC`` records, one per row of ``chunks``), ``box_srcs``
    (stop - first, per_box) rows of ``srcs`` per box (-1 = unused) and ``pool_elems``."""

    def __init__(self, first, stop, chunks, stacks, srcs, box_srcs, pool_elems):
        self.first, self.stop, self.chunks, self.stacks = first, stop, chunks, stacks
        self.srcs, self.box_srcs, self.pool_elems = srcs, box_srcs, pool_elems


def _extent(idx, shape, chunk):
    return tuple(min(c, s - int(i) * c) for i, s, c in zip(idx, shape, chunk))


def _build_group(first, stop, ids, box_ids, shape, chunk, grid, nominal):
    """``ids``: the group's touched chunk ids, ascending (raster order); ``box_ids``: those of each of its boxes."""
    gy, gx = grid[1], grid[2]
    chunks = np.array([(i // (gy * gx), i // gx % gy, i % gx) for i in ids], dtype=np.int64).reshape(-1, 3)
    classes = {}                                    # (truncated z, y, x) -> rows of `chunks`, raster order
    for m, idx in enumerate(chunks):
        ext = _extent(idx, shape, chunk)
        classes.setdefault(tuple(e < c for e, c in zip(ext, chunk)), []).append(m)
    srcs = np.zeros(len(ids), dtype=_native.BOX_SRC)
    stacks, at = [], 0
    for key, rows in classes.items():
        # a class full on some axis stacks along the first such axis; the corner chunk stands alone
        for members in ([rows] if not all(key) else [[m] for m in rows]):
            ext = _extent(chunks[members[0]], shape, chunk)
            axis = key.index(False) if not all(key) else 0
            vshape = list(ext)
            if not all(key):
                vshape[axis] = len(members) * chunk[axis]
            vshape = tuple(vshape)
            dchunk = tuple(chunk) if nominal else tuple(min(c, v) for c, v in zip(chunk, vshape))
            base = -(-at // POOL_ALIGN) * POOL_ALIGN
            at = base + vshape[0] * vshape[1] * vshape[2]
            strides = (vshape[1] * vshape[2], vshape[2], 1)
            for k, m in enumerate(members):
                rec = srcs[m]
                rec["base"] = base + k * chunk[axis] * strides[axis]
                rec["stride_z"], rec["stride_y"] = strides[0], strides[1]
                rec["z0"], rec["y0"], rec["x0"] = (int(i) * c for i, c in zip(chunks[m], chunk))
                rec["ez"], rec["ey"], rec["ex"] = ext
            stacks.append(Stack(vshape, dchunk, axis, list(members), base))
    row_of = {i: m for m, i in enumerate(ids)}
    per_box = max([len(b) for b in box_ids] + [1])
    box_srcs = np.full((stop - first, per_box), -1, dtype=np.int32)
    for n, b in enumerate(box_ids):
        box_srcs[n, :len(b)] = [row_of[i] for i in b]
    return Group(first, stop, chunks, stacks, srcs, box_srcs, at)


def plan_read(shape3, chunk3, starts, box, nominal, max_pool_bytes=1 << 30):
    """The plan of reading N boxes of shape ``box`` at ``starts`` (N, 3; any integers, inside the array or not) from
    an array of ``shape3`` in chunks of ``chunk3``: a list of ``Group``.  ``nominal``: the store's streams keep the
    nominal chunk shape (the bounded formats) instead of the chunk clamped to the array (``exac``).  Boxes go into
    consecutive groups whose decoded chunks (2 bytes a voxel, deduplicated within the group) and table rows (12 + 4
    per touched chunk bytes a box) fit ``max_pool_bytes``; a group holds at least one box, so a cap below one box's
    needs gives one group per box.  The cap covers the decoded chunks and those rows only: neither the up to 256 bytes
    of padding in front of each of a group's at most 8 stacks nor the caller's output is counted."""
    shape = tuple(int(s) for s in shape3)
    chunk = tuple(int(c) for c in chunk3)
    box = tuple(int(b) for b in box)
    if len(shape) != 3 or len(chunk) != 3 or len(box) != 3 or min(shape) < 1 or min(chunk) < 1 or min(box) < 1:
        raise ValueError("plan_read: shape, chunk and box are three positive sizes each")
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

    def nbytes(i):
        e = _extent((i // (grid[1] * grid[2]), i // grid[2] % grid[1], i % grid[2]), shape, chunk)
        return 2 * e[0] * e[1] * e[2]

    groups, first, held, held_bytes, box_ids = [], 0, set(), 0, []
    for n in range(len(starts)):
        ids = ids_of(n)
        own = 12 + 4 * len(ids)                     # the box's start and source list lie on the device too
        more = own + sum(nbytes(i) for i in ids if i not in held)
        if n > first and held_bytes + more > max_pool_bytes:
            groups.append(_build_group(first, n, sorted(held), box_ids, shape, chunk, grid, nominal))
            first, held, held_bytes, box_ids = n, set(), 0, []
            more = own + sum(nbytes(i) for i in ids)
        held.update(ids)
        held_bytes += more
        box_ids.append(ids)
    if len(starts):
        groups.append(_build_group(first, len(starts), sorted(held), box_ids, shape, chunk, grid, nominal))
    return groups


class DevicePatches:
    """A batch of patches that stayed on the device: ``buf`` (a ``DeviceBuffer``; None for an empty batch),
    ``shape`` (N, z, y, x) and ``dtype``.  ``data_ptr()`` makes it an operand of the batched entries."""

    def __init__(self, buf, shape, dtype):
        self.buf, self.shape, self.dtype = buf, tuple(shape), np.dtype(dtype)

    def data_ptr(self):
        return int(self.buf.ptr) if self.buf is not None and self.buf.ptr else 0

    def download(self):
        if self.buf is None:
            return np.empty(self.shape, dtype=self.dtype)
        return self.buf.download(self.shape, self.dtype)

    def free(self):
        if self.buf is not None:
            self.buf.free()


def _axis_range(entry, length):
    """(start, stop, keeps its axis) of one entry of a basic index along an axis of ``length``."""
    if isinstance(entry, slice):
        if entry.step not in (None, 1):
            raise IndexError("StoredArray: slices of step 1 only")
        start, stop, _ = entry.indices(length)
        return start, max(stop, start), True
    if isinstance(entry, (bool, np.bool_, np.ndarray)) or entry is None or entry is Ellipsis:
        raise IndexError("StoredArray: an index is made of integers and step-1 slices")
    try:
        i = operator.index(entry)
    except TypeError:
        raise IndexError("StoredArray: an index is made of integers and step-1 slices") from None
    if not -length <= i < length:
        raise IndexError(f"index {i} is out of bounds for an axis of size {length}")
    i += length if i < 0 else 0
    return i, i + 1, False


def normalize_key(key, shape):
    """A numpy basic index of integers and step-1 slices into an array of ``shape`` -> ``(starts, stops, result
    shape)``; ``IndexError`` for anything else (steps, ``Ellipsis``, ``None``, arrays, too many entries)."""
    key = key if isinstance(key, tuple) else (key,)
    if len(key) > len(shape):
        raise IndexError(f"too many indices: the array is {len(shape)}-dimensional, but {len(key)} were given")
    key = key + (slice(None),) * (len(shape) - len(key))
    ranges = [_axis_range(k, n) for k, n in zip(key, shape)]
    return ([r[0] for r in ranges], [r[1] for r in ranges], tuple(r[1] - r[0] for r in ranges if r[2]))


class StoredArray:
    """A stored (1, 1, z, y, x) uint16 volume read by regions (``chunk_store.open_zarr``) and, opened with
    ``mode="r+"`` (or made by ``chunk_store.create_zarr``), written by regions (``utils/store_write.py``)."""

    ndim = 5
    dtype = np.dtype(np.uint16)

    def __init__(self, path, device=None, max_pool_bytes=1 << 30, mode="r", codec=None):
        if mode not in ("r", "r+"):
            raise ValueError("StoredArray: mode is 'r' or 'r+'")
        with open(os.path.join(path, "zarr.json")) as f:
            self.meta = json.load(f)
        shape3, chunk3, typesize, self._nominal = chunk_store.check_metadata(self.meta)
        if typesize != 2:
            raise NotImplementedError("region reads of int32 (index) stores are not implemented")
        entry = self.meta["codecs"][0]
        if codec is not None and (not isinstance(codec, chunk_store.CODECS[entry["name"]]) or
                                  codec.config_entry() != entry["configuration"]):
            raise ValueError("open_zarr: the codec passed is not the one the store was written with")
        self.path = path
        self.shape = (1, 1) + shape3
        self.chunks = (1, 1) + chunk3
        self.device = device
        self.max_pool_bytes = int(max_pool_bytes)
        self.mode = mode
        self._codec = chunk_store._codec_of(self.meta)
        self._codec.device = device
        # the coder of a write: the stored entry's (an exac store keeps its format version), or the one passed --
        # a block-bounded store with a bound table does not hold the table
        self._write_codec = codec if codec is not None else chunk_store._encoder_of(self.meta)
        if mode == "r+" and codec is None and "bound" in entry["configuration"]:
            raise ValueError("open_zarr: a block-bounded store with a bound table is written with codec=, the "
                             "codec that holds the table")
        self.last_read = None
        self.last_write = None

    def __len__(self):
        return 1

    def __setitem__(self, key, value):
        """``arr[0, 0, z0:z1, y0:y1, x0:x1] = value`` (the indexing rules of ``normalize_key``): ``value`` is an
        array of exactly the result shape, or a scalar; integers in 0..65535 are stored as they are, floats are
        clipped and rounded like ``write_patches``' float32 patches."""
        from aind_exaspim_image_compression.utils import store_write
        store_write.setitem(self, key, value)

    def write_patches(self, voxels, patches, is_center=True, offset=0.0, mask=None):
        """Writes (N, z, y, x) ``patches`` at ``voxels`` (N, 3), placed as ``read_patches`` places them, in order:
        where patches overlap the later one wins, as in ``for n: arr[box n] = patches[n]``; parts outside the array
        are dropped.  ``patches``: a host uint16 array, a host float32 array (stored as ``rint(clip(v + offset, 0,
        65535))``, computed on the device) or a ``DevicePatches`` of either type, which never visits the host.
        ``mask`` (block-bounded stores only; the patches' shape) marks the voxels held to the codec's
        ``fg_max_error``; without one every voxel is background.

        Only the touched chunks are decoded, changed and coded again; a chunk without a file counts
        as zeros (the fill value), and a chunk file is replaced atomically.  Boxes go into groups under
        ``max_pool_bytes`` and nothing of a group is written before all of it has been coded.  A lossy store
        (``exac-dctq``, ``exac-dctq-block``) takes only writes that cover every touched chunk whole -- aligned to the
        chunk grid or the array's edge -- and raises ``ValueError`` otherwise, before anything is written.
        ``last_write`` describes the last write that succeeded (chunks, chunk_bytes, decoded, encode_calls, groups,
        seconds per phase) and is ``None`` after one that failed.  Concurrent writers to one chunk are undefined:
        each reads, changes and replaces the whole chunk."""
        from aind_exaspim_image_compression.utils import store_write
        store_write.write_patches(self, voxels, patches, is_center=is_center, offset=offset, mask=mask)

    def __getitem__(self, key):
        starts, stops, shape = normalize_key(key, self.shape)
        if 0 in shape or any(b <= a for a, b in zip(starts, stops)):
            return np.empty(shape, dtype=np.uint16)
        box = tuple(b - a for a, b in zip(starts[2:], stops[2:]))
        return self.read_patches([starts[2:]], box, is_center=False)[0].reshape(shape)

    def read_patches(self, voxels, patch_shape, is_center=True, dtype=np.uint16, offset=0.0, fill=0, out="host"):
        """(N, *patch_shape) patches at ``voxels`` (N, 3): box n starts at ``voxel - d // 2`` per axis (the
        reference's ``get_slices``), or at ``voxel`` with ``is_center=False``; voxels outside the array are
        ``fill``.  ``dtype``: uint16, or float32 = value - ``offset`` (``read_counts``).  ``out="device"`` returns a
        ``DevicePatches``.  ``max_pool_bytes`` bounds the decoded chunks held at a time, not the output, which is
        one device allocation of the whole batch.  ``last_read`` describes the last call that succeeded in full; a
        read that fails after it began (a missing or rejected chunk) leaves it ``None``."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint16), np.dtype(np.float32)):
            raise ValueError("read_patches: dtype is uint16 or float32")
        if dt == np.uint16 and float(offset) != 0.0:
            raise ValueError("read_patches: an offset goes with float32 only")
        if dt == np.uint16 and not (float(fill).is_integer() and 0 <= fill <= 65535):
            raise ValueError("read_patches: a uint16 fill must be an integer in 0..65535")
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
        # "seconds": host clock around the file reads, the uploads + decodes (each synchronises) and the gather + its
        # synchronisation, summed over the groups (the pool allocation counts as decode)
        self.last_read = {"chunks": 0, "chunk_bytes": 0, "decode_calls": 0, "groups": 0,
                          "seconds": {"files": 0.0, "decode": 0.0, "gather": 0.0}}
        if n == 0:
            return np.empty(shape, dtype=dt) if out == "host" else DevicePatches(None, shape, dt)
        groups = plan_read(self.shape[2:], self.chunks[2:], starts, box, self._nominal, self.max_pool_bytes)
        ctx = _native.context(self.device)
        box_bytes = box[0] * box[1] * box[2] * dt.itemsize
        d_out = ctx.alloc(n * box_bytes)
        try:
            for g in groups:
                self._read_group(ctx, g, starts, box, dt, offset, fill, int(d_out.ptr) + g.first * box_bytes)
            if out == "device":
                res, d_out = DevicePatches(d_out, shape, dt), None
                return res
            return d_out.download(shape, dt)
        except BaseException:
            self.last_read = None                   # a failed read is not described
            raise
        finally:
            if d_out is not None:
                d_out.free()

    def _read_group(self, ctx, g, starts, box, dt, offset, fill, out_ptr):
        t0 = time.perf_counter()
        blobs = []
        for iz, iy, ix in g.chunks:
            with open(os.path.join(self.path, chunk_store.chunk_key(iz, iy, ix)), "rb") as f:
                blobs.append(f.read())
        t1 = time.perf_counter()
        pool = ctx.alloc(2 * g.pool_elems) if g.pool_elems else None
        try:
            for st in g.stacks:
                data, offsets, sizes = chunk_store.pack_streams([blobs[m] for m in st.members])
                enc = EncodedVolume(data, offsets, sizes, st.shape, st.chunk, 2)
                self._codec.decode_device(ctx, enc, int(pool.ptr) + 2 * st.base)       # synchronises
            t2 = time.perf_counter()
            ctx.gather_boxes(pool, g.pool_elems, g.srcs, g.box_srcs, starts[g.first:g.stop], box, out_ptr, dt,
                             offset, fill)
            ctx.sync()                              # the gather reads the pool: done before it is released
            t3 = time.perf_counter()
        finally:
            if pool is not None:
                pool.free()
        for name, dt_s in (("files", t1 - t0), ("decode", t2 - t1), ("gather", t3 - t2)):
            self.last_read["seconds"][name] += dt_s
        self.last_read["chunks"] += len(blobs)
        self.last_read["chunk_bytes"] += sum(len(b) for b in blobs)
        self.last_read["decode_calls"] += len(g.stacks)
        self.last_read["groups"] += 1
