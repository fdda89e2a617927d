"""The host plan of ``inference.predict_store``: a stored volume cut into bricks of whole destination chunks, and for
each brick the patches of ``predict``'s tiling whose cores meet it and the window of the source they read
(DESIGN.md 5.16).  Pure Python: nothing here touches a device.

Along one axis of ``dim`` voxels ``predict`` runs the patches ``i`` in ``[0, n)``, ``n = len(range(0, dim - patch +
stride, stride))`` and ``stride = patch - overlap``; patch ``i`` reads ``[i * stride, i * stride + patch)`` (zeros
beyond the volume) and adds its core ``[i * stride + trim, i * stride + trim + core)``, ``core = patch - 2 * trim``, cut
at ``dim``.  A brick whose output interval is ``[o0, o1)`` therefore needs exactly the ``i`` with ``i * stride + trim <
o1`` and ``i * stride + trim + core > o0``: a run of consecutive indices, so a brick's patches are a regular grid.
"""
import itertools
from typing import NamedTuple

# Device bytes a brick costs while it is in flight (``Brick.cost``), so that ``plan_predict`` can hold bricks under a
# budget:
WINDOW_BYTES = 2            # per voxel of the brick's input window as it is held (``window_slabs``): the uint16 counts
PRED_BYTES = 4              # per voxel of every patch of the brick: the fp32 predictions kept until they are stitched
BATCH_BYTES = 4             # per voxel of the ``batch_size`` patches of the network's input tensor
BRICK_BYTES = 2             # per voxel of the brick: the stitched uint16 counts
POOL_BYTES = 8              # per voxel of the brick: the destination pool and its coded streams, as
                            # ``bm4d.denoise_store`` counts them (``_STORE_CORE_BYTES``)
READER_SHARE = 8            # the source reader's pool of decoded chunks is capped at budget // READER_SHARE


class Brick(NamedTuple):
    """One brick: ``origin`` / ``extent`` (z, y, x) of its output box, ``first`` / ``count`` the patch indices it
    needs per axis (``count`` may hold a 0: no patch at all), ``win_origin`` / ``win_extent`` the box of the source
    its patches read inside the volume (extent 0 without patches) and ``cost`` in device bytes."""

    origin: tuple
    extent: tuple
    first: tuple
    count: tuple
    win_origin: tuple
    win_extent: tuple
    cost: int

    @property
    def n_patches(self):
        return self.count[0] * self.count[1] * self.count[2]


def window_slabs(wz, chunk_z):
    """``(slabs, slab)``: how a window of ``wz`` layers is read -- ``slabs`` consecutive boxes of ``slab`` layers, about
    a destination chunk each, so that the reader can group them under its pool cap.  The boxes of one read have one
    shape, so the window held is ``slabs * slab`` layers, fewer than ``slabs`` more than ``wz``; the cost counts them."""
    if wz == 0:
        return 0, 0
    slabs = -(-wz // chunk_z)
    return slabs, -(-wz // slabs)


def axis_patches(dim, patch, overlap):
    """The number of patches ``predict`` runs along an axis of ``dim`` voxels."""
    stride = patch - overlap
    return len(range(0, dim - patch + stride, stride))


def patch_range(o0, o1, dim, patch, overlap, trim):
    """``(first, count)`` of the patch indices whose cores meet ``[o0, o1)`` along an axis of ``dim`` voxels."""
    stride, core = patch - overlap, patch - 2 * trim
    lo = max(0, (o0 - trim - core) // stride + 1)                     # i * stride + trim + core > o0
    hi = min(axis_patches(dim, patch, overlap), -(-(o1 - trim) // stride))      # i * stride + trim < o1
    return (lo, hi - lo) if hi > lo else (0, 0)


def _axis(o0, o1, dim, patch, overlap, trim):
    """(first, count, window start, window extent) of one axis of a brick."""
    first, count = patch_range(o0, o1, dim, patch, overlap, trim)
    if count == 0:
        return 0, 0, 0, 0
    stride = patch - overlap
    w0 = first * stride
    return first, count, w0, min((first + count - 1) * stride + patch, dim) - w0


def _held(window, chunk_z):
    """The window as it is held on the device: its z extent rounded up to whole slabs."""
    slabs, slab = window_slabs(window[0], chunk_z)
    return (slabs * slab, window[1], window[2])


def _cost(extent, count, window, patch, batch_size, budget):
    """``window``: as held."""
    pv = patch ** 3
    vox = extent[0] * extent[1] * extent[2]
    return (WINDOW_BYTES * window[0] * window[1] * window[2] + PRED_BYTES * pv * count[0] * count[1] * count[2] +
            BATCH_BYTES * pv * batch_size + (BRICK_BYTES + POOL_BYTES) * vox + budget // READER_SHARE)


def _runs(dim, step):
    return [(o, min(o + step, dim)) for o in range(0, dim, step)]


def plan_predict(shape, chunks_zyx, patch_size, overlap, trim, batch_size, budget_bytes):
    """The bricks of a volume of ``shape`` (z, y, x) stored in destination chunks of ``chunks_zyx``, in raster order.

    Every brick is a box of whole chunks (cut at the volume's faces), all bricks have one shape in chunks, and the
    bricks partition the volume; no destination chunk lies in two bricks, so none is ever read back.

    The shape, deterministic: start from one chunk and grow by one chunk at a time along the axis on which the brick
    is shortest in voxels (the first such axis on a tie), as long as that axis has chunks left and the dearest brick
    of the grown shape stays within ``budget_bytes``; an axis that cannot grow any more is left out and the others
    go on, so bricks stay as cubic as the chunk shape and the volume allow.  The dearest brick is bounded from
    above by taking, per axis, the largest extent, window (as held: ``window_slabs``) and patch count any brick has
    there -- the cost is monotone in each -- which makes the rule cheap for any grid.  A brick of a single chunk is accepted whatever it
    costs."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    patch, overlap, trim, batch_size, budget = (int(patch_size), int(overlap), int(trim), int(batch_size),
                                                int(budget_bytes))
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_predict: shape and chunks are three positive sizes each")
    if batch_size < 1 or not overlap < patch or patch - 2 * trim < 1 or trim < 0 or budget < 1:
        raise ValueError("plan_predict: batch_size >= 1, overlap < patch_size, 0 <= trim, patch_size - 2 trim >= 1 and "
                         "budget_bytes >= 1")
    grid = [-(-s // c) for s, c in zip(shape, chunk)]

    def axes(a, n):
        """The bricks' (o0, o1, first, count, w0, wn) along axis a when a brick is n chunks long."""
        return [(o0, o1) + _axis(o0, o1, shape[a], patch, overlap, trim) for o0, o1 in _runs(shape[a], n * chunk[a])]

    def bound(per_axis):
        return _cost([max(r[1] - r[0] for r in ax) for ax in per_axis], [max(r[3] for r in ax) for ax in per_axis],
                     [max(_held((r[5], 0, 0), chunk[0])[0] if a == 0 else r[5] for r in ax)
                      for a, ax in enumerate(per_axis)], patch, batch_size, budget)

    n = [1, 1, 1]
    per_axis = [axes(a, 1) for a in range(3)]
    open_axes = [a for a in range(3) if grid[a] > 1]
    while open_axes:
        a = min(open_axes, key=lambda a: (min(n[a] * chunk[a], shape[a]), a))
        grown = axes(a, n[a] + 1)
        if bound(per_axis[:a] + [grown] + per_axis[a + 1:]) > budget:
            open_axes.remove(a)
            continue
        n[a] += 1
        per_axis[a] = grown
        if n[a] >= grid[a]:
            open_axes.remove(a)

    bricks = []
    for rz, ry, rx in itertools.product(*per_axis):
        r = (rz, ry, rx)
        extent = tuple(q[1] - q[0] for q in r)
        count = tuple(q[3] for q in r)
        if 0 in count:
            first, count, w0, wn = (0, 0, 0), tuple(count), (0, 0, 0), (0, 0, 0)
        else:
            first, w0, wn = tuple(q[2] for q in r), tuple(q[4] for q in r), tuple(q[5] for q in r)
        bricks.append(Brick(tuple(q[0] for q in r), extent, first, count, w0, wn,
                            _cost(extent, count, _held(wn, chunk[0]), patch, batch_size, budget)))
    return bricks
