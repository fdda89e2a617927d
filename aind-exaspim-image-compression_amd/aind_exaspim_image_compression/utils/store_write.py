"""Region writes of a chunk store: boxes and patch batches that re-code only the chunks they touch.

The mirror of ``utils/store_read.py``, in three separable steps:

* ``plan_write`` (host, numpy) finds the chunks N boxes touch, says of each whether the write covers it whole
  (``covered``), whether its stored contents are needed (``decode``) or whether the fill value 0 supplies the rest
  (``zero``), lays the chunks out as stacks in one pool (``store_read._build_group``: the layout the decode and encode
  entries take unchanged) and lists, per chunk, the boxes that may touch it;
* ``open_pool`` allocates a group's pool, zeroes it where a chunk is ``zero`` and decodes the ``decode`` chunks into
  it; ``scatter`` copies boxes of one device buffer into the pool (``exabm4d_scatter_boxes_dev``, ``csrc/
  region_kernels.hip``) and may be called once per source buffer;
* ``encode_commit`` codes every stack with one ``encode_device`` call and then -- only then -- replaces the chunk
  files, each through a temporary name in its directory and ``os.replace``: a file is always the old or the new stream.

``StoredArray.write_patches`` / ``__setitem__`` run the three per group; ``bm4d.denoise_store`` scatters the cores of
several denoised window batches into one pool before it is coded.
"""
import os
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume
from aind_exaspim_image_compression.utils.store_read import POOL_ALIGN, DevicePatches, _build_group, _extent

COVERED, DECODE, ZERO = "covered", "decode", "zero"


class WriteGroup:
    """Boxes ``[first, stop)`` of a write plan and the chunks they touch: ``chunks`` (M, 3) chunk indices (the
    ``decode`` ones first, raster order within each part), ``states`` (M of "covered" / "decode" / "zero"),
    ``stacks`` (``store_read.Stack``; ``decode_stacks`` of them, the first ones, hold exactly the ``decode`` chunks),
    ``dsts`` (M ``_native.BOX_SRC`` records: where each chunk lies in the pool), ``dst_boxes`` (M, per_dst) the
    boxes that may touch each chunk, numbered from ``first`` and ascending (-1 = unused), and ``pool_elems``."""

    def __init__(self, first, stop, chunks, states, stacks, decode_stacks, dsts, dst_boxes, pool_elems):
        self.first, self.stop, self.chunks, self.states, self.stacks = first, stop, chunks, states, stacks
        self.decode_stacks, self.dsts, self.dst_boxes, self.pool_elems = decode_stacks, dsts, dst_boxes, pool_elems


def _build_write_group(first, stop, held, shape, chunk, grid, nominal, exists, written):
    """``held``: {chunk id: [(box, covers the chunk), ...]} of the group's boxes, in box order."""
    def state(i):
        if any(c for _, c in held[i]):
            return COVERED
        idx = (i // (grid[1] * grid[2]), i // grid[2] % grid[1], i % grid[2])
        return DECODE if i in written or exists is None or exists(*idx) else ZERO

    states = {i: state(i) for i in held}
    parts = [sorted(i for i in held if states[i] == DECODE), sorted(i for i in held if states[i] != DECODE)]
    # the chunks to decode get stacks of their own, so that whole stacks decode into the pool as on the read side
    a = _build_group(first, stop, parts[0], [], shape, chunk, grid, nominal)
    b = _build_group(first, stop, parts[1], [], shape, chunk, grid, nominal)
    shift = -(-a.pool_elems // POOL_ALIGN) * POOL_ALIGN
    for st in b.stacks:
        st.base += shift
        st.members = [m + len(parts[0]) for m in st.members]
    b.srcs["base"] += np.uint64(shift)
    ids = parts[0] + parts[1]
    per_dst = max([len(held[i]) for i in ids] + [1])
    dst_boxes = np.full((len(ids), per_dst), -1, dtype=np.int32)
    for m, i in enumerate(ids):
        dst_boxes[m, :len(held[i])] = [n - first for n, _ in held[i]]
    return WriteGroup(first, stop, np.concatenate([a.chunks, b.chunks]), [states[i] for i in ids],
                      a.stacks + b.stacks, len(a.stacks), np.concatenate([a.srcs, b.srcs]), dst_boxes,
                      shift + b.pool_elems if parts[1] else a.pool_elems)


def plan_write(shape3, chunk3, starts, box, nominal, exists=None, max_pool_bytes=1 << 30):
    """The plan of writing N boxes at ``starts`` (N, 3; any integers) into an array of ``shape3`` in chunks of
    ``chunk3``: a list of ``WriteGroup``.  ``box``: one shape for all boxes, or (N, 3) extents; the parts of a box
    outside the array are dropped.  ``exists(iz, iy, ix)`` says whether a chunk is stored (None: every chunk is); a
    touched chunk is ``covered`` when one box alone covers its whole extent, else ``decode`` when it is stored (or an
    earlier group of this plan writes it), else ``zero``.  Boxes go into consecutive groups under ``max_pool_bytes``
    by ``plan_read``'s rule (2 bytes a voxel of the group's chunks, 12 + 4 per touched chunk bytes a box; at least one
    box a group).  The groups are meant to be executed in order: a chunk two groups touch is read, modified and
    written twice, which keeps the order of ``for n: arr[box n] = v[n]``."""
    shape = tuple(int(s) for s in shape3)
    chunk = tuple(int(c) for c in chunk3)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_write: shape and chunk are three positive sizes each")
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    ext = np.asarray(box, dtype=np.int64)
    if ext.shape not in ((3,), (len(starts), 3)) or (ext.size and ext.min() < 1):
        raise ValueError("plan_write: box is three positive sizes, for all boxes or for each")
    ext = np.broadcast_to(ext, starts.shape)
    grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
    lo_v, hi_v = np.maximum(starts, 0), np.minimum(starts + ext, np.array(shape))     # the box inside the array
    inside = np.all(hi_v > lo_v, axis=1)
    lo, hi = lo_v // np.array(chunk), (hi_v - 1) // np.array(chunk)

    def touched(n):
        """[(chunk id, box n covers it)] in raster order."""
        if not inside[n]:
            return []
        res = []
        for iz in range(lo[n, 0], hi[n, 0] + 1):
            for iy in range(lo[n, 1], hi[n, 1] + 1):
                for ix in range(lo[n, 2], hi[n, 2] + 1):
                    org = (iz * chunk[0], iy * chunk[1], ix * chunk[2])
                    e = _extent((iz, iy, ix), shape, chunk)
                    covers = all(lo_v[n, a] <= org[a] and hi_v[n, a] >= org[a] + e[a] for a in range(3))
                    res.append(((iz * grid[1] + iy) * grid[2] + ix, covers))
        return res

    def nbytes(i):
        e = _extent((i // (grid[1] * grid[2]), i // grid[2] % grid[1], i % grid[2]), shape, chunk)
        return 2 * e[0] * e[1] * e[2]

    groups, first, held, held_bytes, written = [], 0, {}, 0, set()

    def close(stop):
        groups.append(_build_write_group(first, stop, held, shape, chunk, grid, nominal, exists, written))
        written.update(held)

    for n in range(len(starts)):
        t = touched(n)
        own = 12 + 4 * len(t)
        more = own + sum(nbytes(i) for i, _ in t if i not in held)
        if n > first and held_bytes + more > max_pool_bytes:
            close(n)
            first, held, held_bytes = n, {}, 0
            more = own + sum(nbytes(i) for i, _ in t)
        for i, covers in t:
            held.setdefault(i, []).append((n, covers))
        held_bytes += more
    if len(starts):
        close(len(starts))
    return groups


def box_records(starts, box, base=0):
    """``BOX_SRC`` records of N whole boxes of shape ``box`` stored one after another from element ``base``."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    rec = np.zeros(len(starts), dtype=_native.BOX_SRC)
    n = int(box[0]) * int(box[1]) * int(box[2])
    rec["base"] = base + np.arange(len(starts), dtype=np.uint64) * np.uint64(n)
    rec["stride_z"], rec["stride_y"] = int(box[1]) * int(box[2]), int(box[2])
    rec["z0"], rec["y0"], rec["x0"] = starts[:, 0], starts[:, 1], starts[:, 2]
    rec["ez"], rec["ey"], rec["ex"] = (int(b) for b in box)
    return rec


def check_lossy(arr, groups):
    """A lossy store takes whole chunks only: re-coding decoded voxels would let them drift past the bound."""
    if not arr._nominal:
        return
    for g in groups:
        for idx, st in zip(g.chunks, g.states):
            if st != COVERED:
                raise ValueError("a write into a lossy (%s) store must cover every chunk it touches whole: chunk %s is "
                                 "written in part (align the write to the chunk grid or the array's edge)"
                                 % (arr.meta["codecs"][0]["name"], tuple(int(i) for i in idx)))


class Pool:
    """A group's chunks on the device: ``buf`` (uint16, ``elems`` elements) and, where the codec takes a mask and
    one is written, ``mask`` (uint8, the same layout, zero = background)."""

    def __init__(self, buf, mask, elems):
        self.buf, self.mask, self.elems = buf, mask, elems

    def free(self):
        for b in (self.buf, self.mask):
            if b is not None:
                b.free()


def _new_stats():
    return {"chunks": 0, "chunk_bytes": 0, "decoded": 0, "encode_calls": 0, "groups": 0,
            "seconds": {"files_read": 0.0, "decode": 0.0, "scatter": 0.0, "encode": 0.0, "files_write": 0.0}}


def open_pool(arr, ctx, g, stats, want_mask=False):
    """Step 2a: the group's pool, zero where a chunk is ``zero``, the ``decode`` chunks decoded into it."""
    t0 = time.perf_counter()
    blobs = {}
    for m, (idx, st) in enumerate(zip(g.chunks, g.states)):
        if st == DECODE:
            with open(os.path.join(arr.path, chunk_store.chunk_key(*idx)), "rb") as f:
                blobs[m] = f.read()
    t1 = time.perf_counter()
    pool = Pool(ctx.alloc(2 * g.pool_elems), None, g.pool_elems)
    try:
        if ZERO in g.states:
            pool.buf.zero()
        if want_mask:
            pool.mask = ctx.alloc(g.pool_elems).zero()
        for st in g.stacks[:g.decode_stacks]:
            data, offsets, sizes = chunk_store.pack_streams([blobs[m] for m in st.members])
            enc = EncodedVolume(data, offsets, sizes, st.shape, st.chunk, 2)
            arr._codec.decode_device(ctx, enc, int(pool.buf.ptr) + 2 * st.base)       # synchronises
    except BaseException:
        pool.free()
        raise
    stats["seconds"]["files_read"] += t1 - t0
    stats["seconds"]["decode"] += time.perf_counter() - t1
    stats["decoded"] += len(blobs)
    return pool


def scatter(ctx, g, pool, src, src_elems, src_dtype, boxes, dst_boxes=None, offset=0.0, mask=False):
    """Step 2b: boxes of the device buffer ``src`` (``boxes``: their ``BOX_SRC`` records) into the pool -- or, with
    ``mask``, bytes into the mask pool.  ``dst_boxes``: the group's lists in terms of ``boxes`` (default: as
    planned).  Asynchronous."""
    lists = g.dst_boxes if dst_boxes is None else dst_boxes
    if mask:
        ctx.scatter_boxes(src, src_elems, np.uint8, boxes, pool.mask, pool.elems, np.uint8, g.dsts, lists)
    else:
        ctx.scatter_boxes(src, src_elems, src_dtype, boxes, pool.buf, pool.elems, np.uint16, g.dsts, lists, offset)


def replace_chunk_file(final, blob):
    """Replace a chunk file atomically: ``blob`` goes to a temporary name in the file's directory and then takes the
    file's name (``os.replace``), so the file is always the old or the new stream."""
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


def commit_coded_brick(who, out, brick, chunk3, enc):
    """The streams of a coded brick (``enc``: an ``EncodedVolume`` of ``brick.extent`` in chunks of ``chunk3``, the
    brick a box of whole chunks of ``out``) as the chunk files of ``out``, each replaced atomically.  Returns the bytes
    written."""
    first = [o // c for o, c in zip(brick.origin, chunk3)]
    grid = [-(-e // c) for e, c in zip(brick.extent, chunk3)]
    if len(enc.sizes) != grid[0] * grid[1] * grid[2]:
        raise RuntimeError("%s: encode_device returned another number of chunks than the brick holds" % who)
    total = k = 0
    for iz in range(grid[0]):
        for iy in range(grid[1]):
            for ix in range(grid[2]):
                blob = enc.chunk_bytes(k)
                replace_chunk_file(out._chunk_path((first[0] + iz, first[1] + iy, first[2] + ix)), blob)
                total += len(blob)
                k += 1
    return total


def encode_commit(arr, ctx, g, pool, stats, d_table=None):
    """Step 3: every stack coded with one ``encode_device`` call, then the chunk files replaced.  Nothing is written
    before every stack of the group has been coded.  Returns the bytes written."""
    t0 = time.perf_counter()
    codec = arr._write_codec
    blobs = [None] * len(g.chunks)
    for st in g.stacks:
        d_vol = int(pool.buf.ptr) + 2 * st.base
        if codec.takes_mask:
            d_mask = int(pool.mask.ptr) + st.base if pool.mask is not None else None
            enc = codec.encode_device(ctx, d_vol, st.shape, st.chunk, d_mask=d_mask, d_table=d_table)
        else:
            enc = codec.encode_device(ctx, d_vol, st.shape, st.chunk)
        if len(enc.sizes) != len(st.members):
            raise RuntimeError("encode_device returned another number of chunks than the stack holds")
        for k, m in enumerate(st.members):
            blobs[m] = enc.chunk_bytes(k)
    t1 = time.perf_counter()
    total = 0
    for idx, blob in zip(g.chunks, blobs):
        replace_chunk_file(os.path.join(arr.path, chunk_store.chunk_key(*idx)), blob)
        total += len(blob)
    stats["seconds"]["encode"] += t1 - t0
    stats["seconds"]["files_write"] += time.perf_counter() - t1
    stats["chunks"] += len(blobs)
    stats["chunk_bytes"] += total
    stats["encode_calls"] += len(g.stacks)
    stats["groups"] += 1
    return total


def bound_table_on_device(arr, ctx):
    """The write codec's bound table on the device, or None."""
    table = getattr(arr._write_codec, "bound_table", None)
    return None if table is None else ctx.to_device(table)


def _chunk_exists(arr):
    return lambda iz, iy, ix: os.path.exists(os.path.join(arr.path, chunk_store.chunk_key(iz, iy, ix)))


def write_patches(arr, voxels, patches, is_center=True, offset=0.0, mask=None):
    """``StoredArray.write_patches``: see there."""
    arr.last_write = None
    if arr.mode != "r+":
        raise ValueError("the array was opened read-only (open_zarr(path, mode='r+') opens it writable)")
    on_device = isinstance(patches, DevicePatches)
    host = None if on_device else np.asarray(patches)
    shape, dt = (patches.shape, patches.dtype) if on_device else (host.shape, host.dtype)
    if dt not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise ValueError("write_patches: patches are uint16 or float32")
    if dt == np.uint16 and float(offset) != 0.0:
        raise ValueError("write_patches: an offset goes with float32 only")
    if len(shape) != 4 or (shape[0] and min(shape[1:]) < 1):
        raise ValueError("write_patches: patches are (N, z, y, x)")
    box = tuple(int(d) for d in shape[1:])
    starts = np.asarray(voxels)
    if starts.size and not np.issubdtype(starts.dtype, np.integer):
        if not (np.issubdtype(starts.dtype, np.floating) and np.all(starts == np.rint(starts))):
            raise ValueError("write_patches: voxels are integer coordinates")
    starts = starts.astype(np.int64).reshape(-1, 3)
    if len(starts) != shape[0]:
        raise ValueError("write_patches: %d voxels for %d patches" % (len(starts), shape[0]))
    if is_center:
        starts = starts - np.array([d // 2 for d in box])
    if starts.size and (starts.min() < -2 ** 31 or (starts + np.array(box)).max() >= 2 ** 31):
        raise ValueError("write_patches: a box outside the int32 coordinate range")
    codec = arr._write_codec
    if mask is not None:
        if not codec.takes_mask:
            raise ValueError("only a block-bounded store takes a mask")
        mask = np.asarray(mask)
        if mask.shape != tuple(shape):
            raise ValueError("write_patches: the mask has the patches' shape")
        mask = np.ascontiguousarray(mask != 0, dtype=np.uint8)
    stats = _new_stats()
    if len(starts) == 0:
        arr.last_write = stats
        return
    groups = plan_write(arr.shape[2:], arr.chunks[2:], starts, box, arr._nominal, _chunk_exists(arr),
                        arr.max_pool_bytes)
    check_lossy(arr, groups)                         # from the plan alone, before a device is touched
    ctx = _native.context(arr.device)
    n_elems = int(np.prod(shape))
    records = box_records(starts, box)
    held = []
    try:
        d_src = patches if on_device else ctx.to_device(np.ascontiguousarray(host))
        if not on_device:
            held.append(d_src)
        d_mask = None
        if mask is not None:
            d_mask = ctx.to_device(mask)
            held.append(d_mask)
        d_table = bound_table_on_device(arr, ctx)
        if d_table is not None:
            held.append(d_table)
        for g in groups:
            if not len(g.chunks):
                continue
            pool = open_pool(arr, ctx, g, stats, want_mask=d_mask is not None)
            try:
                t0 = time.perf_counter()
                scatter(ctx, g, pool, d_src, n_elems, dt, records[g.first:g.stop], offset=offset)
                if d_mask is not None:
                    scatter(ctx, g, pool, d_mask, n_elems, np.uint8, records[g.first:g.stop], mask=True)
                ctx.sync()
                stats["seconds"]["scatter"] += time.perf_counter() - t0
                encode_commit(arr, ctx, g, pool, stats, d_table)
            finally:
                pool.free()
        arr.last_write = stats
    finally:
        for d in held:
            d.free()


def setitem(arr, key, value):
    """``StoredArray.__setitem__``: see there."""
    from aind_exaspim_image_compression.utils.store_read import normalize_key
    arr.last_write = None
    if arr.mode != "r+":
        raise ValueError("the array was opened read-only (open_zarr(path, mode='r+') opens it writable)")
    starts, stops, shape = normalize_key(key, arr.shape)
    v = np.asarray(value)
    if v.ndim and v.shape != shape:
        raise ValueError("could not assign an array of shape %s to a region of shape %s" % (v.shape, shape))
    if v.dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
        if np.issubdtype(v.dtype, np.integer) or v.dtype == np.bool_:
            if v.size and (v.min() < 0 or v.max() > 65535):
                raise ValueError("values outside the uint16 range")
            v = v.astype(np.uint16)
        elif np.issubdtype(v.dtype, np.floating):
            v = v.astype(np.float32)
        else:
            raise ValueError("values are numbers")
    if 0 in shape or any(b <= a for a, b in zip(starts, stops)):
        arr.last_write = _new_stats()
        return
    box = tuple(b - a for a, b in zip(starts[2:], stops[2:]))
    v = np.broadcast_to(v, box) if v.ndim == 0 else v.reshape(box)
    write_patches(arr, [starts[2:]], np.ascontiguousarray(v)[np.newaxis], is_center=False)
