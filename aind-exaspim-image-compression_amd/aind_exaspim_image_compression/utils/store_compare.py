"""The host side of ``evaluate.compare_stores``: the brick plan of scoring one stored volume against
another, and what follows on the host from the signed difference table the device builds.  Pure Python and numpy:
nothing here touches a device.

A brick is a box of whole chunks of the reference store's grid.  Its *window* is what has to be read to score it:
the brick grown per axis by the SSIM window's reach -- ``left = window // 2`` below, ``window - left - 1`` above --
where indices past a face of the volume stand for their scipy "reflect" images inside it; an axis shorter than the
SSIM window is read whole.
"""
import itertools
import math
from typing import NamedTuple

import numpy as np

from aind_exaspim_image_compression.utils.store_predict import READER_SHARE, _runs, window_slabs

DIFF_BINS = 131071          # the signed difference table: bin (test - ref) + 65535
WINDOW_BYTES = 2            # per voxel of a window as it is held (``window_slabs``), for every store read


class Brick(NamedTuple):
    """One brick: ``origin`` / ``extent`` (z, y, x) of the box that is scored, ``win_origin`` / ``win_extent`` the box
    of the volume its SSIM needs, and ``cost`` in device bytes."""

    origin: tuple
    extent: tuple
    win_origin: tuple
    win_extent: tuple
    cost: int

    @property
    def window_voxels(self):
        return self.win_extent[0] * self.win_extent[1] * self.win_extent[2]


def halo_range(b0, bd, dim, window):
    """``(start, extent)`` of the smallest interval of an axis of ``dim`` voxels that holds every sample the SSIM of
    the voxels ``[b0, b0 + bd)`` reads: the indices ``b0 - left .. b0 + bd - 1 + window - left - 1``, reflected."""
    if dim < window:
        return 0, dim
    left = window // 2
    lo_raw, hi_raw = b0 - left, b0 + bd - 1 + window - left - 1
    lo, hi = max(lo_raw, 0), min(hi_raw, dim - 1)
    if lo_raw < 0:                                  # the indices -1 .. lo_raw stand for 0 .. -lo_raw - 1
        hi = max(hi, -lo_raw - 1)
    if hi_raw >= dim:                               # dim .. hi_raw stand for dim - 1 .. 2 dim - 1 - hi_raw
        lo = min(lo, 2 * dim - 1 - hi_raw)
    return lo, hi - lo + 1


def _cost(windows_held, stores, budget, window_bytes=WINDOW_BYTES):
    """``windows_held``: the window as held, (z, y, x)."""
    return stores * (window_bytes * windows_held[0] * windows_held[1] * windows_held[2] + budget // READER_SHARE)


def _held_z(wz, chunk_z):
    slabs, slab = window_slabs(wz, chunk_z)
    return slabs * slab


def plan_compare(shape, chunks_zyx, window, budget_bytes, with_mask=False):
    """The bricks of scoring a volume of ``shape`` (z, y, x) whose reference store has chunks of ``chunks_zyx``, in
    raster order, for an SSIM window of ``window`` voxels.

    Every brick is a box of whole chunks (cut at the volume's faces), all bricks have one shape in chunks, and they
    partition the volume.  The shape is found as ``store_predict.plan_predict`` finds it: start from one chunk and
    grow by a chunk along the axis on which the brick is shortest in voxels (the first such axis on a tie), as long as
    that axis has chunks left and the dearest brick of the grown shape stays within ``budget_bytes``; an axis that
    cannot grow is left out and the others go on.  A brick costs the windows of the two stores (three
    ``with_mask``) at 2 bytes a voxel, as they are held -- read in z slabs of about a chunk (``window_slabs``), so up
    to a slab count of layers more than the window -- plus each store's pool of decoded chunks, capped at
    ``budget_bytes // READER_SHARE``.  The dearest brick is bounded by the largest window any brick has per axis.  A
    brick of a single chunk is accepted whatever it costs."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    window, budget, stores = int(window), int(budget_bytes), 3 if with_mask else 2
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_compare: shape and chunks are three positive sizes each")
    if not 1 <= window <= 32 or budget < 1:
        raise ValueError("plan_compare: 1 <= window <= 32 and budget_bytes >= 1")
    return plan_bricks(shape, chunk, budget, stores, lambda b0, bd, dim: halo_range(b0, bd, dim, window))


def plan_bricks(shape, chunk, budget, stores, axis_window, brick_bytes=0, window_bytes=WINDOW_BYTES, fixed_bytes=0):
    """``plan_compare``'s rule for any window: ``axis_window(b0, bd, dim) -> (start, extent)`` is what a brick that
    covers ``[b0, b0 + bd)`` of an axis of ``dim`` voxels has to read there; ``stores`` windows are held at a time.
    ``brick_bytes``: what a loop holds besides the windows, per voxel of the brick itself (a result, a pool of
    destination chunks); ``window_bytes``: what it holds per voxel of a window as held, the window itself included;
    ``fixed_bytes``: and per brick.  ``axis_window`` may also be three such functions, one per axis (z, y, x): a
    window in other coordinates than the bricks', as a pyramid level's in its source (``store_pyramid``)."""
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    windows = tuple(axis_window) if isinstance(axis_window, (tuple, list)) else (axis_window,) * 3

    def axes(a, n):
        """The bricks' (o0, o1, w0, wn) along axis a when a brick is n chunks long."""
        return [(o0, o1) + tuple(windows[a](o0, o1 - o0, shape[a])) for o0, o1 in _runs(shape[a], n * chunk[a])]

    def bound(per_axis):
        widest = [max(r[3] for r in ax) for ax in per_axis]
        longest = [max(r[1] - r[0] for r in ax) for ax in per_axis]
        return (_cost((_held_z(widest[0], chunk[0]), widest[1], widest[2]), stores, budget, window_bytes) +
                brick_bytes * longest[0] * longest[1] * longest[2] + fixed_bytes)

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
    for r in itertools.product(*per_axis):
        wn = tuple(q[3] for q in r)
        ext = tuple(q[1] - q[0] for q in r)
        bricks.append(Brick(tuple(q[0] for q in r), ext, tuple(q[2] for q in r), wn,
                            _cost((_held_z(wn[0], chunk[0]), wn[1], wn[2]), stores, budget, window_bytes) +
                            brick_bytes * ext[0] * ext[1] * ext[2] + fixed_bytes))
    return bricks


# ---- what follows from the signed difference table ---------------------------------------------------------------
def _table(error_hist):
    h = np.asarray(error_hist)
    if h.shape != (DIFF_BINS,):
        raise ValueError("a signed difference table has %d bins" % DIFF_BINS)
    return h


def error_stats(error_hist, data_range=None):
    """``{"n", "mae", "mse", "bias", "lmax"}`` (and ``"psnr"`` with a ``data_range``) of the errors counted in a signed
    difference table: the sums are Python integers, exact for any number of voxels, and each mean is one float64
    division of two of them.  ``psnr`` is ``10 log10(data_range^2 / mse)``, ``inf`` without an error; an empty
    table gives ``nan`` means and ``lmax`` 0."""
    h = _table(error_hist)
    bins = np.nonzero(h)[0]
    n = s_abs = s_sq = s = lmax = 0
    for b in bins.tolist():
        c, d = int(h[b]), b - 65535
        n += c
        s += c * d
        s_abs += c * abs(d)
        s_sq += c * d * d
        lmax = max(lmax, abs(d))
    if n == 0:
        out = {"n": 0, "mae": float("nan"), "mse": float("nan"), "bias": float("nan"), "lmax": 0}
    else:
        out = {"n": n, "mae": s_abs / n, "mse": s_sq / n, "bias": s / n, "lmax": lmax}
    if data_range is not None:
        mse = out["mse"]
        out["psnr"] = float("inf") if mse == 0 else 10.0 * math.log10(float(data_range) ** 2 / mse)
    return out


def abs_error_percentile(error_hist, q):
    """The ``q``-th percentile (0..100) of ``|error|`` over the voxels counted in a signed difference table: what
    ``np.percentile(np.abs(test - ref), q)`` gives with its default linear rule -- the order statistics at
    ``floor`` and ``ceil`` of ``(n - 1) q / 100`` and numpy's interpolation between them -- found from the cumulative
    counts, so for any number of voxels below 2^53."""
    h = _table(error_hist).astype(np.uint64)
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError("percentiles lie in 0..100")
    folded = h[65535:].copy()
    folded[1:] += h[65534::-1]
    cum = np.cumsum(folded, dtype=np.uint64)
    n = int(cum[-1])
    if n == 0:
        return float("nan")
    pos = (n - 1) * (q / 100.0)                       # numpy's virtual index, in float64 as there
    below = math.floor(pos)
    t = pos - below
    lo_rank, hi_rank = int(below), min(int(below) + 1, n - 1)
    a = float(np.searchsorted(cum, np.uint64(lo_rank), side="right"))       # the value of 0-based rank lo_rank
    b = float(np.searchsorted(cum, np.uint64(hi_rank), side="right"))
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)
