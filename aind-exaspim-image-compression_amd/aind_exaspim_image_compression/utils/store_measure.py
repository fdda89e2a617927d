"""The host side of ``utils.noise.measure_store``: the wide noise table and how the table of every
shift follows from it, the brick plan of measuring a stored volume, and what follows on the host from the two integer
tables the device builds.  Pure Python and numpy: nothing here touches a device.

The wide table.  For uint16 data a cell's ``m = |d| <= 4 * 65535 < 2^18``.  ``m < 4096`` has the wide bin ``m``;
otherwise, with ``j = floor(log2 m) - 11`` (1..6), the bin ``4096 + (j - 1) 2048 + ((m >> j) - 2048)``: 4096 + 6 * 2048
= 16384 bins a level, each exact below 4096 and 11 significant bits wide above.  Wide bin ``w`` starts at ``v0(w)`` --
``w`` below 4096, otherwise ``(2048 + r) << j`` with ``j = (w - 4096) // 2048 + 1`` and ``r = (w - 4096) % 2048`` -- and
the table at shift ``k`` is ``hist_k[level][min(v0(w) >> k, 4095)] += wide[level][w]``, exactly: an octave ``j <= k``
is at least as fine as ``2^k``, and an octave ``j > k`` holds only ``m >= 4096 << k``, the last bin.  So one pass over
the volume serves ``noise_table``'s rule for choosing the shift, which in memory repeats the pass.

A brick is a box of whole chunks.  Its *window* is the brick extended per axis on the high side to the next even
coordinate (cut at the volume's face): a 2x2x2 cell of the volume's even grid is counted by the brick that holds its
origin, and its far corner may lie one voxel outside that brick.
"""
from dataclasses import dataclass

import numpy as np

from aind_exaspim_image_compression.utils import order_stats, store_compare

LEVELS = 49                 # _native.NOISE_LEVELS
BINS = 4096                 # _native.NOISE_BINS
WIDE_BINS = 16384           # _native.NOISE_WIDE_BINS
COUNT_BINS = 65536          # _native.COUNT_BINS
MAX_SHIFT = 6
M_MAX = 4 * 65535


# ---- the wide table ----------------------------------------------------------------------------------------------
def wide_bin(m):
    """The wide bin of ``m = |d|`` (array or scalar, 0..4 * 65535)."""
    m = np.asarray(m, dtype=np.int64)
    if m.size and (m.min() < 0 or m.max() > M_MAX):
        raise ValueError("wide_bin: |d| of uint16 data lies in 0..%d" % M_MAX)
    big = np.maximum(m, BINS)
    j = np.floor(np.log2(big.astype(np.float64))).astype(np.int64) - 11     # exact: big < 2^18
    return np.where(m < BINS, m, BINS + (j - 1) * 2048 + ((big >> j) - 2048))


def wide_low_value(w):
    """``v0(w)``: the lowest ``m`` of wide bin ``w`` (array or scalar, 0..16383)."""
    w = np.asarray(w, dtype=np.int64)
    if w.size and (w.min() < 0 or w.max() >= WIDE_BINS):
        raise ValueError("wide_low_value: a wide bin lies in 0..%d" % (WIDE_BINS - 1))
    over = np.maximum(w - BINS, 0)
    return np.where(w < BINS, w, (2048 + over % 2048) << (over // 2048 + 1))


def fold_noise_table(wide, shift):
    """``(LEVELS, BINS)`` uint64: the noise table at ``shift`` (0..6) of the cells counted in the wide table ``wide``
    ``(LEVELS, WIDE_BINS)``."""
    wide = np.asarray(wide)
    if wide.shape != (LEVELS, WIDE_BINS):
        raise ValueError("a wide noise table has %d x %d bins" % (LEVELS, WIDE_BINS))
    if not 0 <= int(shift) <= MAX_SHIFT:
        raise ValueError("shift must be 0..%d" % MAX_SHIFT)
    to = np.minimum(wide_low_value(np.arange(WIDE_BINS)) >> int(shift), BINS - 1)
    hist = np.zeros((LEVELS, BINS), dtype=np.uint64)
    np.add.at(hist, (np.arange(LEVELS)[:, None], to[None, :]), wide.astype(np.uint64))
    return hist


# ---- the brick plan ----------------------------------------------------------------------------------------------
def cell_window(b0, bd, dim):
    """``(start, extent)`` along an axis of ``dim`` voxels of what the brick ``[b0, b0 + bd)`` reads: itself, and the
    voxel behind it when it ends at an odd coordinate inside the volume."""
    end = b0 + bd
    return b0, min(end + (end & 1), dim) - b0


def plan_measure(shape, chunks_zyx, budget_bytes, with_mask=False):
    """The bricks (``store_compare.Brick``) of measuring a volume of ``shape`` (z, y, x) stored in chunks of
    ``chunks_zyx``, in raster order.

    Every brick is a box of whole chunks (cut at the volume's faces), all bricks have one shape in chunks, they
    partition the volume, and the shape is grown as ``store_compare.plan_compare`` grows it.  A brick's window is
    ``cell_window`` per axis.  A brick costs its window at 2 bytes a voxel as it is held (in z slabs of about a chunk)
    for the store, and for the mask store ``with_mask``, plus each reader's pool of decoded chunks, capped at
    ``budget_bytes // READER_SHARE``.  A brick of a single chunk is accepted whatever it costs."""
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunks_zyx)
    budget = int(budget_bytes)
    if len(shape) != 3 or len(chunk) != 3 or min(shape) < 1 or min(chunk) < 1:
        raise ValueError("plan_measure: shape and chunks are three positive sizes each")
    if budget < 1:
        raise ValueError("plan_measure: budget_bytes >= 1")
    return store_compare.plan_bricks(shape, chunk, budget, 2 if with_mask else 1, cell_window)


# ---- what follows from the tables --------------------------------------------------------------------------------
def _counts(a, name):
    a = np.asarray(a)
    if a.shape != (COUNT_BINS,):
        raise ValueError("%s has %d counters" % (name, COUNT_BINS))
    return a.astype(np.uint64)


def _twice_median(table):
    """The sum of the two middle values of the population that holds the value ``i`` ``table[i]`` times."""
    cum = np.cumsum(table, dtype=np.uint64)
    n = int(cum[-1])
    lo = np.searchsorted(cum, np.uint64((n - 1) // 2 + 1))
    hi = np.searchsorted(cum, np.uint64(n // 2 + 1))
    return int(lo) + int(hi)


def cut_of_threshold(thr):
    """The least integer count above the threshold ``thr`` (counts), clamped to 0..65536."""
    thr = float(thr)
    if np.isnan(thr):
        raise ValueError("a foreground threshold is a number")
    if thr < 0.0:
        return 0
    if thr >= COUNT_BINS - 1:
        return COUNT_BINS
    return int(np.floor(thr)) + 1


@dataclass
class StoreMeasure:
    """What one pass over a uint16 volume leaves: ``counts[v]`` voxels of every value, the wide noise table
    ``noise_wide`` ``(LEVELS, WIDE_BINS)`` of its 2x2x2 cells and their ``sum_s`` per level; measured with a mask also
    each of them for the foreground (``_fg``) and the background (``_bg``) alone -- a voxel where its mask says, a cell
    in the background only if all eight of its voxels are -- with the plain fields their sums.  Every estimator below
    is host scalar work on these integers and gives what its in-memory namesake gives on the whole array."""

    shape: tuple
    counts: np.ndarray
    noise_wide: np.ndarray
    sum_s: np.ndarray
    counts_fg: np.ndarray = None
    counts_bg: np.ndarray = None
    noise_wide_fg: np.ndarray = None
    noise_wide_bg: np.ndarray = None
    sum_s_fg: np.ndarray = None
    sum_s_bg: np.ndarray = None

    def __post_init__(self):
        self.shape = tuple(int(s) for s in self.shape)
        self.counts = _counts(self.counts, "counts")
        if int(self.counts.sum()) != self.shape[0] * self.shape[1] * self.shape[2]:
            raise ValueError("StoreMeasure: the counts do not add up to the volume's voxels")

    @classmethod
    def from_tables(cls, shape, counts, noise):
        """From the downloaded device tables: ``counts`` ``(tables, COUNT_BINS)`` and ``noise`` ``(tables, LEVELS *
        WIDE_BINS + LEVELS)``, one table each or two (foreground, background)."""
        counts = np.asarray(counts, dtype=np.uint64).reshape(-1, COUNT_BINS)
        noise = np.asarray(noise, dtype=np.uint64).reshape(counts.shape[0], LEVELS * WIDE_BINS + LEVELS)
        wide = noise[:, :LEVELS * WIDE_BINS].reshape(-1, LEVELS, WIDE_BINS)
        sum_s = noise[:, LEVELS * WIDE_BINS:]
        if counts.shape[0] == 1:
            return cls(shape, counts[0], wide[0], sum_s[0])
        return cls(shape, counts[0] + counts[1], wide[0] + wide[1], sum_s[0] + sum_s[1], counts[0], counts[1], wide[0],
                   wide[1], sum_s[0], sum_s[1])

    # -- the counts -------------------------------------------------------------------------------
    @property
    def masked(self):
        return self.counts_fg is not None

    @property
    def n(self):
        return int(self.counts.sum())

    @property
    def min(self):
        return int(np.nonzero(self.counts)[0][0])

    @property
    def max(self):
        return int(np.nonzero(self.counts)[0][-1])

    @property
    def zero_fraction(self):
        return 1.0 - (self.n - int(self.counts[0])) / self.n

    def offset(self, percentile=1.0, ignore_zeros=True):
        """``transforms.estimate_offset`` of the volume."""
        stats = order_stats.from_u16_hist(self.counts, ignore_zeros=ignore_zeros, dtype=np.float32)
        return float(order_stats.percentile(stats, percentile))

    def background_offset_statistics(self, percentile=0.1):
        """``transforms.background_offset_statistics`` of the volume."""
        from aind_exaspim_image_compression.machine_learning.transforms import background_offset_statistics_of_hist
        return background_offset_statistics_of_hist(self.counts, percentile)

    # -- the foreground threshold ------------------------------------------------
    def foreground_threshold(self, k=6.0):
        """``make_foreground_mask``'s threshold ``med + k * 1.4826 * (MAD + 1e-6)`` of the whole volume as the
        ``np.float32`` numpy's fp32 arithmetic gives, from the counts alone.  The median of integer counts is the mean
        of the two middle ones, a multiple of 1/2 and exact in fp32; the deviations ``|v - med|`` are then exact as
        well, and their median is that of the counts folded onto ``|2 v - 2 med|``, halved.  The four operations that
        follow round to fp32 one by one (``order_stats`` works in fp64 and differs after the ``+ 1e-6``)."""
        k = float(k)
        if not np.isfinite(k) or k < 0.0:
            raise ValueError("foreground_threshold: k must be finite and >= 0")
        med2 = _twice_median(self.counts)
        folded = np.zeros(2 * (COUNT_BINS - 1) + 1, dtype=np.uint64)
        np.add.at(folded, np.abs(2 * np.arange(COUNT_BINS, dtype=np.int64) - med2), self.counts)
        mad4 = _twice_median(folded)
        f32 = np.float32
        med = f32(med2) / f32(2)
        mad = f32(mad4) / f32(4) + f32(1e-6)
        sigma = f32(1.4826) * mad
        with np.errstate(over="ignore"):
            return f32(med + f32(k) * sigma)

    def foreground_cut(self, k=6.0):
        """The least count above ``foreground_threshold(k)``, 0..65536: for integer counts ``raw > thr`` is
        ``raw >= cut``, and a cut of 65536 means that no voxel is foreground."""
        return cut_of_threshold(self.foreground_threshold(k))

    # -- the noise table --------------------------------------------------------------------------
    def _wide(self, which):
        if which == "all":
            return self.noise_wide, self.sum_s
        if which not in ("fg", "bg"):
            raise ValueError("which is 'all', 'fg' or 'bg', not %r" % (which,))
        if not self.masked:
            raise ValueError("which=%r needs a measurement with a mask" % which)
        return (self.noise_wide_fg, self.sum_s_fg) if which == "fg" else (self.noise_wide_bg, self.sum_s_bg)

    def noise_table(self, shift=None, min_cells=512, which="all"):
        """``noise.noise_table`` of the volume as a ``noise.NoiseTable``: folded from the wide table at ``shift``, or
        with ``shift=None`` at the smallest shift at which the table is not ``saturated(min_cells)`` -- the rule for
        which the in-memory function repeats its pass.  ``which``: all cells, or with a mask the foreground's or the
        background's alone."""
        from aind_exaspim_image_compression.utils.noise import NoiseTable
        wide, sum_s = self._wide(which)
        if shift is not None:
            return NoiseTable(fold_noise_table(wide, shift), np.array(sum_s, dtype=np.uint64), 0, int(shift))
        for k in range(MAX_SHIFT + 1):
            table = NoiseTable(fold_noise_table(wide, k), np.array(sum_s, dtype=np.uint64), 0, k)
            if not table.saturated(min_cells):
                break
        return table

    def sigma(self, which="all"):
        """``noise.estimate_sigma`` of the volume."""
        return self.noise_table(which=which).pooled_sigma()

    def noise_curve(self, min_cells=512, which="all"):
        """``noise.noise_curve`` of the volume: (mean_counts, sigma, cells) per usable level."""
        from aind_exaspim_image_compression.utils.noise import _curve
        return _curve(self.noise_table(min_cells=min_cells, which=which), min_cells)

    def poisson_gaussian(self, offset=None, min_cells=512, which="all"):
        """``noise.estimate_poisson_gaussian`` of the volume; ``offset`` defaults to ``self.offset()``."""
        from aind_exaspim_image_compression.utils.noise import fit_poisson_gaussian
        if offset is None:
            offset = self.offset()
        return fit_poisson_gaussian(*self.noise_curve(min_cells, which), offset)

    def anscombe_cfg(self, **kw):
        """``noise.anscombe_cfg`` of the volume."""
        return {"kind": "anscombe", "params": self.poisson_gaussian(**kw)}
