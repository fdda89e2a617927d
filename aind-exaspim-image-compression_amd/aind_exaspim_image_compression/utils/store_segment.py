"""The connected components of a stored volume, out of core, as a label store: ``components_store``
labels the seeds of the whole volume store to store, ``components_volume`` is its in-memory twin.

A brick is labelled inside its WINDOW: the brick grown by one voxel on the high side of every axis, cut at the volume's
faces (``exabm4d_component_seeds_u16_dev`` with box = window).  A window label in volume coordinates -- 1 + the volume
index of the window component's first voxel -- is a PROVISIONAL label.  Pass 1 records, per brick, what joins them
(``exabm4d_segment_collect_dev``, ``csrc/segment_kernels.hip``): the seeds of the window outside the brick (halo
records), the seeds of the brick on a low face that has a brick before it (face records), each with its provisional
label, and per window component the voxels of it inside the brick (size records).  ``merge_records`` joins every halo
record to the face record of the same voxel, unites the labels so joined and takes the minimum of each set.  Pass 2
labels every window again -- the labelling is a pure function of the window -- and writes the brick with the final
labels (``exabm4d_segment_relabel_dev``), coded and committed chunk file by chunk file.

Why the union is complete.  Two adjacent seeds a and b (6- or 26-connectivity) differ by at most one voxel per axis.
Take per axis the lower of their two brick indices: the window of that brick holds both, so they lie in one window
component and carry one provisional label there.  A seed that this brick does not own is a halo voxel of it and lies
on a low face of its owner (the bricks are a grid, so the first voxel past a brick on an axis is the origin of the next
brick on that axis), and its halo record is joined to its owner's face record of the same voxel.  Along a path of
adjacent seeds every step therefore stays within one set.  Raster order inside a window agrees with the volume's,
every provisional label is 1 + the index of a voxel of its component, and the component's first voxel is the first
voxel of the window component of the brick that owns it: the minimum over a set is 1 + the volume index of the
component's first voxel, ``metrics.label_components``' label without its 2^31 limit.
"""
import time

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import store_compare
from aind_exaspim_image_compression.utils.store_foreground import _check_filter_args, _check_mask_args
from aind_exaspim_image_compression.utils.store_measure import StoreMeasure, cut_of_threshold
from aind_exaspim_image_compression.utils.store_windows import PhaseClock

# The byte account of a brick (``plan_segment``), per voxel of its window W and of the brick B:
#   window          2 W    the uint16 counts as read
#   scratch        12 W    the labeller's three 32-bit arrays (exabm4d_components_scratch_bytes); after the labelling
#                          the first is the own-count array of the collection, and in pass 2 the first two are the
#                          window-shaped array of final labels (at most 8 bytes an element)
#   labels          4 W    the uint32 labels of the window
#   halo records   16 (W - B), taken as 16 W: the geometric worst case, every voxel of the window outside the brick
#   face records   16 B    at most: the voxels of the brick on its three low faces
#   size records    1 B    ``SIZE_RECORDS_DIV`` voxels a record of 16 bytes; more are collected in a second go
#   dense output   ts B    the relabelled brick at the destination's typesize
#   coded output   (ts + 1) B  the encoder's bound for chunks of whole 8^3 blocks: raw blocks and their table entries
# Not all of it is held at one time (the window goes before the records come, the records before the output), so the
# account is an upper bound; ``stats["largest_alloc"]`` says what a run held.
SEGMENT_WINDOW_BYTES = 2 + 12 + 4 + 16
SEGMENT_FIXED_BYTES = 3 * 256 + 64          # the scratch's alignment, the counters and the least record buffers
SIZE_RECORDS_DIV = 16                       # a size record is reserved per so many voxels of a brick ...
SIZE_RECORDS_MIN = 4096                     # ... and at least so many


def segment_brick_bytes(typesize):
    """What a brick costs per voxel of the brick itself (the account above)."""
    return 16 + 1 + int(typesize) + int(typesize) + 1


def high_window(b0, bd, dim):
    """``axis_window`` of ``store_compare.plan_bricks``: the brick and one voxel more on the high side, cut at the
    face: ``[b0, min(dim, b0 + bd + 1))``."""
    return b0, min(dim, b0 + bd + 1) - b0


def plan_segment(shape, chunks_zyx, budget_bytes, typesize):
    """The bricks (``store_compare.Brick``) of labelling a volume of ``shape`` (z, y, x) into a label store with
    chunks of ``chunks_zyx`` and elements of ``typesize`` bytes, in raster order: boxes of whole destination chunks
    that partition the volume, grown as ``store_compare.plan_compare`` grows them.  A brick's window is the brick
    grown by one voxel on the high side of each axis only, cut at the volume's faces.  The cost is the account next to
    ``SEGMENT_WINDOW_BYTES`` and the reader's pool of decoded chunks.  A brick of a single chunk is accepted whatever
    it costs.  However large the budget, a window stays under the labeller's 2^31 voxels."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    budget = int(budget_bytes)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_segment: shape and chunks are three positive sizes each")
    if typesize not in (4, 8) or budget < 1:
        raise ValueError("plan_segment: typesize 4 or 8 and budget_bytes >= 1")
    # the labeller takes fewer than 2^31 voxels a window: a budget that such a window would exceed is not spent
    budget = min(budget, SEGMENT_WINDOW_BYTES * (2 ** 31 - 1))
    return store_compare.plan_bricks(shape, chunk, budget, 1, high_window, segment_brick_bytes(typesize),
                                     SEGMENT_WINDOW_BYTES, SEGMENT_FIXED_BYTES)


def _pairs(records):
    r = np.ascontiguousarray(records, dtype=np.uint64)
    if r.size % 2 or (r.ndim > 1 and r.shape[-1] != 2):
        raise ValueError("merge_records: records are pairs of uint64")
    return r.reshape(-1, 2)


def merge_records(halo, face, size):
    """The merge of all bricks' records.  ``halo`` and ``face``: (voxel index, provisional label) pairs; ``size``:
    (provisional label, own voxels) pairs (anything that reshapes to (N, 2) uint64; duplicates of halo and face records
    change nothing).  Every halo record is joined to the face record of the same voxel (``RuntimeError`` where a halo
    voxel has none: the bricks' plan is wrong), the labels so joined are united over all labels seen, and a set's
    representative is its minimum.  Returns ``(keys, vals, table)``: the sorted labels seen with their final labels,
    and the (final label, voxels) table, sorted by label.

    Vectorised: the labels become indices into their sorted list, so the smallest index of a set is its smallest
    label; rounds of hooking (the larger root of an edge under the smaller, ``np.minimum.at``) and pointer jumping to a
    fixed point (``p = p[p]``) run until nothing changes.  No Python loop per record."""
    halo, face, size = _pairs(halo), _pairs(face), _pairs(size)
    keys = np.unique(np.concatenate([size[:, 0], halo[:, 1], face[:, 1]]))
    parent = np.arange(keys.size, dtype=np.int64)
    if halo.shape[0]:
        order = np.argsort(face[:, 0], kind="stable")
        fv, fl = face[order, 0], face[order, 1]
        at = np.searchsorted(fv, halo[:, 0])
        found = at < fv.size
        found[found] = fv[at[found]] == halo[found, 0]
        if not np.all(found):
            raise RuntimeError("merge_records: %d halo voxels have no face record (the first: voxel %d)"
                               % (int(np.count_nonzero(~found)), int(halo[~found, 0][0])))
        # a voxel lies on the low faces of one brick: its face records (duplicates apart) carry one label
        a, b = np.searchsorted(keys, halo[:, 1]), np.searchsorted(keys, fl[at])
        live = a != b
        a, b = a[live], b[live]
        while a.size:
            pa, pb = parent[a], parent[b]
            lo = np.minimum(pa, pb)
            np.minimum.at(parent, pa, lo)
            np.minimum.at(parent, pb, lo)
            while True:                                  # (a chain halves per step: log2 of its length)
                nxt = parent[parent]
                if np.array_equal(nxt, parent):
                    break
                parent = nxt
            live = parent[a] != parent[b]
            a, b = a[live], b[live]
    vals = keys[parent]
    final = vals[np.searchsorted(keys, size[:, 0])]
    order = np.argsort(final, kind="stable")
    final, own = final[order], size[order, 1]
    table = np.zeros((0, 2), dtype=np.uint64)
    if final.size:
        starts = np.flatnonzero(np.concatenate(([True], final[1:] != final[:-1])))
        table = np.stack([final[starts], np.add.reduceat(own, starts)], axis=1).astype(np.uint64)
    return keys, vals, table


def final_labels(table, min_voxels=0, relabel=False):
    """What the components of ``table`` ((label, voxels) sorted by label) become: a uint64 per row -- 0 where the
    component has fewer than ``min_voxels`` voxels, else its label, or with ``relabel`` its rank 1..n among the kept
    ones in that order (``scipy.ndimage.label``'s numbering)."""
    table = np.asarray(table, dtype=np.uint64).reshape(-1, 2)
    kept = table[:, 1] >= np.uint64(max(0, int(min_voxels)))
    out = np.where(kept, table[:, 0], np.uint64(0))
    if relabel:
        out = np.where(kept, np.cumsum(kept, dtype=np.uint64), np.uint64(0))
    return out.astype(np.uint64)


def _size_capacity(voxels):
    return max(int(SIZE_RECORDS_MIN), int(voxels) // int(SIZE_RECORDS_DIV), 1)


def _prod(t):
    return int(t[0]) * int(t[1]) * int(t[2])


class _Run:
    """The two passes over the bricks of one volume.  ``read(brick)`` gives ``(buffer, origin, dims, release)`` of a
    uint16 window on the device that holds the brick's window; ``emit(brick, d_out)`` takes a relabelled brick."""

    def __init__(self, ctx, shape, bricks, cut, connectivity, typesize, read, timed):
        self.ctx, self.shape, self.bricks, self.cut, self.connectivity = ctx, shape, bricks, cut, connectivity
        self.typesize, self.read = typesize, read
        self.clock = PhaseClock(("read", "label", "collect", "merge", "relabel"), timed, ctx.sync)
        self.seconds = self.clock.seconds
        self.most, self.voxels_read, self.repeats = 0, 0, 0
        self.records = {"halo": 0, "face": 0, "size": 0}

    def _label(self, brick):
        """(d_labels, d_scratch) of the brick's window; the caller frees both."""
        ctx = self.ctx
        t0 = time.perf_counter()
        win, w0, wd, release = self.read(brick)
        d_labels = d_scratch = None
        try:
            t1 = self.clock()
            nwin = _prod(brick.win_extent)
            scratch_bytes = max(256, _native.components_scratch_bytes(brick.win_extent, self.connectivity))
            d_scratch = ctx.alloc(scratch_bytes)
            d_labels = ctx.alloc(4 * nwin)
            self.most = max(self.most, 2 * _prod(wd) + scratch_bytes + 4 * nwin)
            ctx.component_seeds_u16(win, self.shape, w0, wd, brick.win_origin, brick.win_extent, self.cut, 1,
                                    self.connectivity, labels=d_labels, scratch=d_scratch)
            t2 = self.clock()
        except BaseException:
            for buf in (d_labels, d_scratch):
                if buf is not None:
                    buf.free()
            raise
        finally:
            release()                                    # (freeing a buffer waits for the stream)
        self.seconds["read"] += t1 - t0
        self.seconds["label"] += t2 - t1
        self.voxels_read += brick.window_voxels
        return d_labels, d_scratch

    def collect(self):
        """Pass 1: (halo, face, size) records of all bricks, and per brick the provisional labels it reported."""
        ctx = self.ctx
        halos, faces, sizes, reported = [], [], [], []
        d_counts = ctx.alloc(24)
        try:
            for brick in self.bricks:
                d_labels, d_scratch = self._label(brick)
                d_halo = d_face = d_size = None
                try:
                    t0 = self.clock()
                    halo_cap, face_cap = _native.segment_record_capacities(brick.win_extent, brick.origin, brick.extent)
                    size_cap = _size_capacity(_prod(brick.extent))
                    d_halo, d_face = ctx.alloc(max(16, 16 * halo_cap)), ctx.alloc(max(16, 16 * face_cap))
                    for attempt in range(2):
                        d_size = ctx.alloc(16 * size_cap)
                        self.most = max(self.most, d_scratch.nbytes + d_labels.nbytes + d_halo.nbytes + d_face.nbytes +
                                        d_size.nbytes + 24)
                        ctx.segment_collect(d_labels, self.shape, brick.win_origin, brick.win_extent, brick.origin,
                                            brick.extent, d_scratch, d_halo, halo_cap, d_face, face_cap, d_size, size_cap,
                                            d_counts)
                        n_halo, n_face, n_size = (int(c) for c in d_counts.download((3,), np.uint64))
                        if n_halo > halo_cap or n_face > face_cap:
                            raise RuntimeError("components: more halo or face records than the geometry allows")
                        if n_size <= size_cap:
                            break
                        if attempt:
                            raise RuntimeError("components: the size records changed between two collections")
                        # all were counted and size_cap of them stored: once more, with room for every one
                        self.repeats += 1
                        d_size.free()
                        d_size, size_cap = None, n_size
                    for d_buf, n, into in ((d_halo, n_halo, halos), (d_face, n_face, faces), (d_size, n_size, sizes)):
                        into.append(d_buf.download((n, 2), np.uint64) if n else np.zeros((0, 2), np.uint64))
                    reported.append(np.sort(sizes[-1][:, 0]))
                    self.records["halo"] += n_halo
                    self.records["face"] += n_face
                    self.records["size"] += n_size
                    self.seconds["collect"] += self.clock() - t0
                finally:
                    for buf in (d_labels, d_scratch, d_halo, d_face, d_size):
                        if buf is not None:
                            buf.free()
        finally:
            d_counts.free()
        return np.concatenate(halos), np.concatenate(faces), np.concatenate(sizes), reported

    def relabel(self, keys, out_vals, reported, emit):
        """Pass 2: every brick with its final labels, handed to ``emit``.  ``out_vals``: per key what it becomes."""
        ctx, ts = self.ctx, self.typesize
        for brick, mine in zip(self.bricks, reported):
            # the brick's slice of the table: the labels it reported whose final value differs or is dropped
            becomes = out_vals[np.searchsorted(keys, mine)] if mine.size else mine
            sel = becomes != mine
            k, v = np.ascontiguousarray(mine[sel]), np.ascontiguousarray(becomes[sel])
            d_labels, d_scratch = self._label(brick)
            d_keys = d_vals = d_out = None
            try:
                t0 = self.clock()
                if k.size:
                    d_keys, d_vals = ctx.to_device(k), ctx.to_device(v)
                d_out = ctx.alloc(ts * _prod(brick.extent))
                self.most = max(self.most, d_scratch.nbytes + d_labels.nbytes + 16 * k.size + d_out.nbytes)
                ctx.segment_relabel(d_labels, self.shape, brick.win_origin, brick.win_extent, brick.origin, brick.extent,
                                    d_keys, d_vals, k.size, ts, d_scratch, d_out)
                self.seconds["relabel"] += self.clock() - t0
                for buf in (d_labels, d_scratch, d_keys, d_vals):
                    if buf is not None:
                        buf.free()
                d_labels = d_scratch = d_keys = d_vals = None
                emit(brick, d_out)
            finally:
                for buf in (d_labels, d_scratch, d_keys, d_vals, d_out):
                    if buf is not None:
                        buf.free()

    def run(self, min_voxels, relabel, emit):
        """Both passes and the merge between them; returns the result's table entries."""
        halo, face, size, reported = self.collect()
        t0 = time.perf_counter()
        keys, vals, table = merge_records(halo, face, size)
        del halo, face, size
        becomes = final_labels(table, min_voxels, relabel)
        if becomes.size and int(becomes.max()) >= 2 ** (8 * self.typesize):
            raise ValueError("components: a label does not fit the destination's uint%d" % (8 * self.typesize))
        out_vals = becomes[np.searchsorted(table[:, 0], vals)] if vals.size else vals
        self.seconds["merge"] += time.perf_counter() - t0
        self.relabel(keys, out_vals, reported, emit)
        kept = becomes != 0
        sizes = table[kept, 1]
        return {"n_seed": int(table[:, 1].sum(dtype=np.uint64)), "n_components": int(table.shape[0]),
                "n_kept_components": int(np.count_nonzero(kept)), "n_kept_voxels": int(sizes.sum(dtype=np.uint64)),
                "largest": int(table[:, 1].max()) if table.shape[0] else 0,
                "labels": becomes[kept].astype(np.uint64), "sizes": sizes.astype(np.uint64)}


def _label_dtype(who, dtype, voxels, relabel):
    """The destination's element size: ``dtype`` (uint32 / uint64), or by the volume's size."""
    if dtype is None:
        return 4 if voxels <= 2 ** 32 - 1 else 8
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt not in (np.dtype(np.uint32), np.dtype(np.uint64)):
        raise ValueError("%s: dtype is uint32 or uint64 (or None)" % who)
    if dt.itemsize == 4 and voxels > 2 ** 32 - 1 and not relabel:
        raise ValueError("%s: the labels of a volume of %d voxels do not fit uint32" % (who, voxels))
    return dt.itemsize


def _check_common(who, k, threshold, measure, connectivity, min_voxels, budget_bytes):
    _check_mask_args(who, k, 0, threshold)
    min_voxels = _check_filter_args(who, min_voxels, connectivity, most=2 ** 63 - 1)
    if measure is not None and not isinstance(measure, StoreMeasure):
        raise ValueError("%s: measure is a StoreMeasure (utils.noise.measure_store)" % who)
    if int(budget_bytes) < 1:
        raise ValueError("%s: budget_bytes must be positive" % who)
    return min_voxels


def components_store(src, dst_path, threshold=None, measure=None, k=6.0, connectivity=26, min_voxels=0, relabel=False,
                     dtype=None, chunks=None, attributes=None, budget_bytes=4 << 30, device=None, stats=None):
    """The connected components of the seeds of the stored uint16 volume ``src`` as a label store, without ever holding
    the volume: ``dst_path`` is, chunk file for chunk file, ``write_zarr(expected.astype(dtype), dst_path, chunks,
    codec=LabelCodec(typesize))`` of the labelling of the whole volume, whatever the brick plan.

    Seeds are the voxels with a count ``>= cut``; the cut is found as ``foreground_store`` finds it: ``threshold`` (a
    number in counts) if given; else ``measure.foreground_cut(k)`` of a ``StoreMeasure`` of ``src``; else the function
    measures ``src`` first (one more pass).  A mask store of ``foreground_store`` is labelled with ``threshold=0``.
    Nothing is dilated.  The label of a component (``connectivity`` 6 or 26) is 1 + the linear (z, y, x) index in the
    whole volume of its first voxel in raster order, background 0 -- ``label_components``' rule without its limit of
    2^31 voxels; ``relabel=True`` renumbers the kept components 1..n in that order (``scipy.ndimage.label``'s
    numbering).  Components of fewer than ``min_voxels`` voxels (any integer >= 0) become 0: the sizes are the whole
    volume's, there is no halo rule and no cap.

    ``dtype``: uint32 or uint64; None is uint32 where the volume has at most 2^32 - 1 voxels, else uint64;
    ``ValueError`` where a label cannot fit.  The destination is made with ``create_zarr`` (``chunks``: default the
    source's; ``LabelCodec(typesize)``; ``attributes``).  Bricks are boxes of whole destination chunks
    (``plan_segment``, at most ``budget_bytes`` of device memory each; a single chunk is taken whatever it costs).
    Two passes over the source (module docstring): per brick a region read of its window, the labelling, and then the
    records of the merge (pass 1) or the relabelled brick, coded by ``LabelCodec.encode_device`` and committed (pass 2).

    Returns ``{"cut", "n", "n_seed", "n_components", "n_kept_components", "n_kept_voxels", "largest", "cratio",
    "labels", "sizes"}``: the voxels, the seeds, the components before and after ``min_voxels``, the voxels of the
    kept ones and of the largest component, raw bytes / stored bytes, and the sorted final labels of the kept
    components with their voxel counts (uint64 each).  ``stats`` (a dict) receives ``seconds`` per phase (measure,
    read, label, collect, merge, relabel, encode, files_write; the stream is synchronised around the phases only when
    ``stats`` is given), ``bricks``, ``passes``, ``voxels_read``, ``largest_alloc``, ``records`` (halo, face, size) and
    ``collect_repeats``, the bricks whose size records took a second collection."""
    from aind_exaspim_image_compression.utils import chunk_store, noise, store_windows, store_write
    from aind_exaspim_image_compression.utils.label_codec import LabelCodec
    who = "components_store"
    # -- every argument check, before a context exists
    min_voxels = _check_common(who, k, threshold, measure, connectivity, min_voxels, budget_bytes)
    budget = int(budget_bytes)
    chunks = store_windows.check_chunks(chunks)
    if dtype is not None:
        _label_dtype(who, dtype, 1, relabel)
    index = int(device) if device is not None else _native.default_device()
    (arr,) = store_windows.open_u16_stores(who, (("src", src),), index)
    shape = tuple(int(s) for s in arr.shape[2:])
    n = shape[0] * shape[1] * shape[2]
    typesize = _label_dtype(who, dtype, n, relabel)
    if measure is not None and threshold is None and tuple(measure.shape) != shape:
        raise ValueError("components_store: measure was made of another shape than src")
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    bricks = plan_segment(shape, chunks[2:], budget, typesize)

    seconds = dict.fromkeys(("measure", "read", "label", "collect", "merge", "relabel", "encode", "files_write"), 0.0)
    passes, measured_voxels, most = 2, 0, 0
    if threshold is not None:
        cut = cut_of_threshold(float(threshold))
    else:
        if measure is None:
            t0 = time.perf_counter()
            inner = {}
            measure = noise.measure_store(arr, budget_bytes=budget, device=index, stats=inner)
            seconds["measure"] = time.perf_counter() - t0
            passes, measured_voxels, most = 3, inner["voxels_read"], inner["largest_alloc"]
        cut = int(measure.foreground_cut(k))

    ctx = _native.context(index)
    codec = LabelCodec(typesize, device=index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    chunk3 = tuple(int(c) for c in chunks[2:])
    source = store_windows.StoreWindows([arr], int(arr.chunks[2]))

    def read(brick):
        wins, dims = source.read(brick.win_origin, brick.win_extent)
        return wins[0], brick.win_origin, dims, lambda: source.release(wins)

    run = _Run(ctx, shape, bricks, cut, connectivity, typesize, read, stats is not None)
    written = [0]

    def emit(brick, d_out):
        t0 = run.clock()
        run.most = max(run.most, d_out.nbytes + _native.label_encode_bound(typesize, brick.extent, codec._chunk(
            brick.extent, chunk3)))
        enc = codec.encode_device(ctx, d_out, brick.extent, chunk3)
        t1 = time.perf_counter()
        written[0] += store_write.commit_coded_brick(who, out, brick, chunk3, enc)
        seconds["encode"] += t1 - t0
        seconds["files_write"] += time.perf_counter() - t1

    with store_windows.capped_pools([arr], budget):
        res = run.run(min_voxels, relabel, emit)
    seconds.update(run.seconds)
    if stats is not None:
        stats.update(seconds=seconds, bricks=len(bricks), passes=passes, voxels_read=run.voxels_read + measured_voxels,
                     largest_alloc=max(most, run.most), records=dict(run.records), collect_repeats=run.repeats)
    return dict(res, cut=cut, n=n, cratio=typesize * n / written[0])


def components_volume(vol_or_mask, threshold=None, measure=None, k=6.0, connectivity=26, min_voxels=0, relabel=False,
                      dtype=None, brick=None, device=None, stats=None):
    """``components_store`` for a 3-D array in memory: ``(labels, table)``, the label array (``dtype``) and the dict
    ``components_store`` returns (without ``cratio``).  A uint16 array is a volume whose seeds are the counts ``>=
    cut`` (``threshold``, else ``measure``, else the table of its own counts); a bool or uint8 array is a mask whose
    non-zero voxels are the seeds.  The array is uploaded once and processed as bricks of shape ``brick`` (z, y, x;
    default: one brick) through the same two passes: the result does not depend on ``brick``."""
    who = "components_volume"
    a = np.asarray(vol_or_mask)
    if a.dtype not in (np.dtype(np.uint16), np.dtype(np.uint8), np.dtype(np.bool_)) or a.ndim != 3 or 0 in a.shape:
        raise ValueError("components_volume: a 3-D uint16 volume or bool / uint8 mask without an empty axis")
    min_voxels = _check_common(who, k, threshold, measure, connectivity, min_voxels, 1)
    shape = tuple(int(s) for s in a.shape)
    n = a.size
    typesize = _label_dtype(who, dtype, n, relabel)
    if brick is not None:
        try:
            brick = tuple(int(b) for b in brick)
        except TypeError:
            brick = ()
        if len(brick) != 3 or min(brick) < 1:
            raise ValueError("components_volume: brick is three positive sizes")
    if measure is not None and threshold is None and tuple(measure.shape) != shape:
        raise ValueError("components_volume: measure was made of another shape than the volume")
    # budget 1: every brick is one "chunk" of shape ``brick``
    bricks = plan_segment(shape, brick if brick is not None else shape, 1, typesize)
    ctx = _native.context(device)
    d_vol = None
    seconds = dict.fromkeys(("measure", "read", "label", "collect", "merge", "relabel", "encode", "files_write"), 0.0)
    try:
        if a.dtype == np.uint16:
            d_vol = ctx.to_device(np.ascontiguousarray(a))
            if threshold is not None:
                cut = cut_of_threshold(float(threshold))
            elif measure is not None:
                cut = int(measure.foreground_cut(k))
            else:
                t0 = time.perf_counter()
                hist = ctx.u16_histogram(d_vol, a.size)
                dummy = np.zeros((1, _native.measure_noise_words()), dtype=np.uint64)
                cut = int(StoreMeasure.from_tables(shape, hist, dummy).foreground_cut(k))
                seconds["measure"] = time.perf_counter() - t0
        else:
            d_vol = ctx.to_device(np.ascontiguousarray(a != 0).astype(np.uint16))
            cut = 1
        labels = np.zeros(shape, dtype=np.uint32 if typesize == 4 else np.uint64)

        def read(b):
            return d_vol, (0, 0, 0), shape, lambda: None

        def emit(b, d_out):
            z, y, x = b.origin
            ez, ey, ex = b.extent
            labels[z:z + ez, y:y + ey, x:x + ex] = d_out.download(b.extent, labels.dtype)

        run = _Run(ctx, shape, bricks, cut, connectivity, typesize, read, stats is not None)
        res = run.run(min_voxels, relabel, emit)
    finally:
        if d_vol is not None:
            d_vol.free()
    seconds.update(run.seconds)
    if stats is not None:
        stats.update(seconds=seconds, bricks=len(bricks), passes=2, voxels_read=run.voxels_read,
                     largest_alloc=run.most + 2 * n, records=dict(run.records), collect_repeats=run.repeats)
    return labels, dict(res, cut=cut, n=n)
