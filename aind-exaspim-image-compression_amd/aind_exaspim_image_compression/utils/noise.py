"""Noise sigma and Poisson-Gaussian parameters measured from the data, on the GPU.

Every BM4D entry point takes its noise level from the caller, and ``AnscombeTransform`` its ``gain`` and
``read_noise``.  This module measures them.  One HIP kernel (``exabm4d_noise_table_dev``, csrc/noise_kernels.hip)
reads the volume once and leaves a small integer table on the host; everything after it is scalar float64 work.

The table.  The volume is cut into 2x2x2 cells at even coordinates.  A cell with voxels v[dz][dy][dx] gives
s = sum v and d = sum (-1)^(dz+dy+dx) v, the unnormalised Haar HHH detail: Var d = 8 sigma^2 for i.i.d. noise, and d
is orthogonal to s.  The cell counts in ``hist[level][min(|d| >> shift, 4095)]``, where ``level`` is the
quarter-octave bin of the cell mean (t = (s >> 3) + 16, e = floor(log2 t), level = 4 (e - 4) + ((t >> (e - 2)) & 3),
0..48), and adds s to ``sum_s[level]``.  The median of |d| over a row, divided by 0.6745 sqrt(8), is a robust sigma
at that intensity; over the sum of all rows it is Donoho's pooled estimator.

Limitation: on cells that lie on sharp structure d carries signal, and the estimate reads high there
(DESIGN.md 5.9 has the numbers).  There is no CPU fallback: without a GPU the functions raise ``NativeError``.
"""
import math
from dataclasses import dataclass

import numpy as np

from aind_exaspim_image_compression import _native

LEVELS = _native.NOISE_LEVELS
BINS = _native.NOISE_BINS
MAX_SHIFT = 6
# median of |N(0, 1)|, times the norm of the eight +-1 weights of d
_MAD_TO_SIGMA = 0.674489750196082 * math.sqrt(8.0)


@dataclass
class NoiseTable:
    """The device's table and what follows from it directly: ``counts[level]`` cells and
    ``means[level] = sum_s / (8 counts)`` in counts (NaN for an empty level)."""

    hist: np.ndarray        # (LEVELS, BINS) uint64
    sum_s: np.ndarray       # (LEVELS,) uint64
    skipped: int            # fp32 cells with a non-finite s or d
    shift: int
    counts: np.ndarray = None
    means: np.ndarray = None

    def __post_init__(self):
        self.counts = self.hist.sum(axis=1, dtype=np.uint64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.means = self.sum_s.astype(np.float64) / (8.0 * self.counts.astype(np.float64))

    def sigma_of(self, hist_row):
        """Interpolated median of |d| over ``hist_row`` (BINS counts), divided by 0.674489750196082 sqrt(8).

        Bin b of width w = 2^shift covers [b w - 0.5, (b + 1) w - 0.5), bin 0 starts at 0.  The median is the
        point where the cumulative count reaches n / 2, linear inside its bin.  NaN for an empty row, and for a
        median in the last bin, which has no upper edge."""
        row = np.asarray(hist_row, dtype=np.uint64)
        cum = np.cumsum(row, dtype=np.uint64)
        n = int(cum[-1])
        if n == 0:
            return float("nan")
        half = n / 2.0
        b = int(np.searchsorted(cum, half, side="left"))
        if b >= BINS - 1:
            return float("nan")
        w = float(1 << self.shift)
        lower = b * w - 0.5 if b else 0.0
        upper = (b + 1) * w - 0.5
        below = float(cum[b - 1]) if b else 0.0
        median = lower + (half - below) / float(row[b]) * (upper - lower)
        return median / _MAD_TO_SIGMA

    def pooled_sigma(self):
        return self.sigma_of(self.hist.sum(axis=0, dtype=np.uint64))

    def saturated(self, min_cells):
        """The pooled row, or a level with at least ``min_cells`` cells, has its median in the last bin."""
        rows = [self.hist.sum(axis=0, dtype=np.uint64)]
        rows += [self.hist[lv] for lv in range(LEVELS) if int(self.counts[lv]) >= min_cells]
        return any(int(r.sum()) > 0 and math.isnan(self.sigma_of(r)) for r in rows)


def _is_device(vol):
    """A ``DeviceBuffer``, a raw device address, or a tensor that lives on a GPU.  A tensor in host memory is a
    host array like any other: its ``data_ptr`` is no address the kernel may read."""
    if isinstance(vol, (_native.DeviceBuffer, int)):
        return True
    return hasattr(vol, "data_ptr") and bool(getattr(vol, "is_cuda", False))


def _resident(vol, shape, dtype, device):
    """(ctx, device buffer, dtype, shape, buffer to free or None) of ``vol`` in HBM, uploaded if it is on the host."""
    from aind_exaspim_image_compression.machine_learning.metrics import DeviceImage
    owned = None
    if isinstance(vol, DeviceImage):
        ctx, buf, dtype, shape = vol.ctx, vol.buf, vol.dtype, vol.shape
    elif _is_device(vol):
        if shape is None or dtype is None:
            raise ValueError("a device buffer needs shape=(nz, ny, nx) or (batch, nz, ny, nx) and dtype=")
        ctx = vol.ctx if isinstance(vol, _native.DeviceBuffer) else _native.context(device)
        buf = vol
    else:
        arr = np.asarray(vol)
        if arr.dtype != np.uint16:
            arr = arr.astype(np.float32, copy=False)
        dtype, shape = arr.dtype, arr.shape
    shape = tuple(int(x) for x in shape)
    dtype = np.dtype(dtype)
    if len(shape) not in (3, 4):
        raise ValueError("noise_table expects a 3-D volume or a 4-D batch of patches")
    if min(shape) < 1 or min(shape[-3:]) < 2:
        raise ValueError("noise_table: every extent must be >= 2")
    if dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise ValueError("noise_table: a resident volume must be uint16 or float32")
    if not (isinstance(vol, DeviceImage) or _is_device(vol)):
        ctx = _native.context(device)
        buf = owned = ctx.to_device(np.ascontiguousarray(arr).reshape(-1))
    return ctx, buf, dtype, shape, owned


def _one_pass(ctx, buf, dtype, shape, shift):
    """The table of a 3-D volume, or of a 4-D batch as ONE population: cells never straddle two patches, so an
    even nz lets the batch go as one volume of batch * nz planes; otherwise the patches' tables are added."""
    if len(shape) == 3 or shape[0] == 1:
        return ctx.noise_table(buf, dtype, shape[-3:], shift)
    b, nz, ny, nx = shape
    if nz % 2 == 0:
        return ctx.noise_table(buf, dtype, (b * nz, ny, nx), shift)
    hist = np.zeros((LEVELS, BINS), dtype=np.uint64)
    sum_s = np.zeros(LEVELS, dtype=np.uint64)
    skipped = 0
    step = nz * ny * nx * np.dtype(dtype).itemsize
    base = _native._ptr(buf)
    for i in range(b):
        h, s, k = ctx.noise_table(base + i * step, dtype, (nz, ny, nx), shift)
        hist += h
        sum_s += s
        skipped += k
    return hist, sum_s, skipped


def noise_table(vol, shift=None, device=None, min_cells=512, shape=None, dtype=None):
    """The noise table of ``vol``: a numpy uint16 or float32 array (other dtypes are converted to float32), 3-D or a
    4-D batch of patches treated as one population (a tensor in host memory counts as such an array); or a
    ``DeviceImage``; or a device buffer / pointer / GPU tensor with ``shape=`` and ``dtype=``, which is read where
    it is.

    ``shift=None`` starts at 0 and repeats the pass with a larger shift while the pooled row, or any level with at
    least ``min_cells`` cells, has its median in the last bin (sigma above about 2100 counts at shift 0)."""
    ctx, buf, dt, shp, owned = _resident(vol, shape, dtype, device)
    try:
        if shift is not None:
            if not 0 <= int(shift) <= MAX_SHIFT:
                raise ValueError("shift must be 0..%d" % MAX_SHIFT)
            return NoiseTable(*_one_pass(ctx, buf, dt, shp, int(shift)), int(shift))
        for k in range(MAX_SHIFT + 1):
            table = NoiseTable(*_one_pass(ctx, buf, dt, shp, k), k)
            if not table.saturated(min_cells):
                break
        return table
    finally:
        if owned is not None:
            owned.free()


def estimate_sigma(vol, device=None, **kw):
    """Noise standard deviation of ``vol`` in its own units: Donoho's pooled estimator, the median of |d| over
    all cells divided by 0.6745 sqrt(8).

    A uint16 volume has been rounded to whole counts, which adds 1/12 to the variance of every voxel; the
    estimate includes it (it reads sqrt(sigma^2 + 1/12) for an analogue noise sigma) and nothing is subtracted:
    that is the noise BM4D meets in the stored data."""
    return noise_table(vol, device=device, **kw).pooled_sigma()


def _curve(table, min_cells):
    keep, sig = [], []
    for lv in range(LEVELS):
        if int(table.counts[lv]) >= max(1, int(min_cells)):
            s = table.sigma_of(table.hist[lv])
            if not math.isnan(s):
                keep.append(lv)
                sig.append(s)
    keep = np.asarray(keep, dtype=np.int64)
    return table.means[keep], np.asarray(sig, dtype=np.float64), table.counts[keep].astype(np.int64)


def noise_curve(vol, min_cells=512, device=None, **kw):
    """(mean_counts, sigma, cells) of the levels with at least ``min_cells`` cells whose median is not in the last
    bin: the noise level as a function of intensity.  ``mean = sum_s / (8 cells)``."""
    return _curve(noise_table(vol, device=device, min_cells=min_cells, **kw), min_cells)


def fit_poisson_gaussian(mean, sigma, cells, offset):
    """Weighted least-squares line sigma^2 = a mean + c; weights cells / sigma^4, because the variance of a
    variance estimate is proportional to sigma^4 / n.  Levels with sigma = 0 carry no finite weight and are left
    out.  gain = a, read_noise = sqrt(max(c + a offset, 0))."""
    mean, sigma, cells = (np.asarray(v, dtype=np.float64) for v in (mean, sigma, cells))
    ok = sigma > 0.0
    mean, sigma, cells = mean[ok], sigma[ok], cells[ok]
    if mean.size < 3:
        raise ValueError("estimate_poisson_gaussian: fewer than three usable intensity levels (%d); the volume "
                         "spans too little intensity, or min_cells is too large" % mean.size)
    y = sigma * sigma
    w = cells / (y * y)
    wsum = np.sum(w)
    xm = np.sum(w * mean) / wsum
    ym = np.sum(w * y) / wsum
    a = np.sum(w * (mean - xm) * (y - ym)) / np.sum(w * (mean - xm) * (mean - xm))
    c = ym - a * xm
    if not a > 0.0:
        raise ValueError("estimate_poisson_gaussian: the fitted slope is not positive (a = %g): the noise does not "
                         "grow with the intensity, so there is no Poisson gain to read" % a)
    return {"gain": float(a), "read_noise": float(math.sqrt(max(c + a * float(offset), 0.0))),
            "offset": float(offset)}


def estimate_poisson_gaussian(vol, offset=None, min_cells=512, device=None, **kw):
    """``{"gain", "read_noise", "offset"}`` of the model counts = gain Poisson(clean / gain) + N(offset,
    read_noise), from the line sigma^2 = gain (mean - offset) + read_noise^2 through the noise curve.  ``offset``
    defaults to ``transforms.estimate_offset(vol)``, for which ``vol`` must be a host array.  Fewer than three
    usable levels, or a slope <= 0, raise ``ValueError``."""
    mean, sigma, cells = noise_curve(vol, min_cells=min_cells, device=device, **kw)
    if offset is None:
        from aind_exaspim_image_compression.machine_learning.metrics import DeviceImage
        from aind_exaspim_image_compression.machine_learning.transforms import estimate_offset
        if isinstance(vol, DeviceImage) or _is_device(vol):
            raise ValueError("estimate_poisson_gaussian: give offset= for a volume that is not a host array")
        offset = estimate_offset(vol)
    return fit_poisson_gaussian(mean, sigma, cells, offset)


def anscombe_cfg(vol, **kw):
    """A transform cfg for ``transforms.build_transform`` with the measured parameters."""
    return {"kind": "anscombe", "params": estimate_poisson_gaussian(vol, **kw)}


# ---- measuring a stored volume out of core ------------------------------------------------------
def _measure(ctx, shape, bricks, source, with_mask, stats):
    """The loop of ``measure_store`` / ``measure_volume`` over ``bricks``; ``source.read(origin, extent)`` gives the
    windows (volume[, mask]) and their extent as held."""
    import time
    from aind_exaspim_image_compression.utils.store_measure import StoreMeasure
    from aind_exaspim_image_compression.utils.store_windows import PhaseClock
    tables = 2 if with_mask else 1
    table_bytes = 8 * tables * (_native.COUNT_BINS + _native.measure_noise_words())
    clock = PhaseClock(("read", "measure", "download"), stats is not None, ctx.sync)
    seconds = clock.seconds
    voxels_read, most = 0, 0
    d_counts = d_noise = None
    try:
        d_counts = ctx.alloc(8 * tables * _native.COUNT_BINS)
        d_noise = ctx.alloc(8 * tables * _native.measure_noise_words())
        for k, brick in enumerate(bricks):
            t0 = time.perf_counter()
            wins, dims = source.read(brick.win_origin, brick.win_extent)
            most = max(most, table_bytes + 2 * len(wins) * dims[0] * dims[1] * dims[2])
            voxels_read += brick.window_voxels
            try:
                t1 = clock()
                ctx.measure_box_u16(wins[0], wins[1] if with_mask else None, shape, brick.win_origin, dims,
                                    brick.origin, brick.extent, d_counts, d_noise, zero_first=k == 0)
                seconds["measure"] += clock() - t1
                seconds["read"] += t1 - t0
            finally:
                source.release(wins)                 # (freeing a buffer waits for the stream)
        t0 = time.perf_counter()
        counts = d_counts.download((tables, _native.COUNT_BINS), np.uint64)
        tab = d_noise.download((tables, _native.measure_noise_words()), np.uint64)
        seconds["download"] += time.perf_counter() - t0
    finally:
        for buf in (d_counts, d_noise):
            if buf is not None:
                buf.free()
    if stats is not None:
        stats.update(seconds=seconds, bricks=len(bricks), voxels_read=voxels_read, largest_alloc=most, passes=1)
    return StoreMeasure.from_tables(shape, counts, tab)


def measure_store(src, mask=None, budget_bytes=4 << 30, device=None, stats=None):
    """Measures the stored uint16 volume ``src`` without ever holding it: what ``measure_volume(read_zarr(src)[0, 0])``
    returns, for a volume of any size.  The ``StoreMeasure`` that comes back gives, as host scalar
    work and bit for bit as the in-memory functions give them on the whole array, ``offset()``
    (``transforms.estimate_offset``), ``background_offset_statistics()``, ``noise_table()``, ``sigma()``
    (``estimate_sigma``), ``noise_curve()``, ``poisson_gaussian()`` (``estimate_poisson_gaussian``) and
    ``anscombe_cfg()`` -- the ``sigma=`` / ``noise=`` of ``bm4d.denoise_store`` and the offset of
    ``inference.build_volume_transform`` for ``predict_store``.

    ``src`` and ``mask`` (non-zero = foreground) are paths or ``StoredArray``s of uint16 and one shape, opened for the
    device used here.  Bricks are boxes of whole chunks of ``src`` (``utils.store_measure.plan_measure``, each at most
    ``budget_bytes`` of device memory; a single chunk is taken whatever it costs).  Per brick one region read per store
    stays on the device and one kernel adds the brick to two integer tables there -- the counts of every value, and a
    wide noise table from which the table of every shift follows -- which are downloaded once at the end.  **Every
    chunk is read and decoded once**, whatever shift the noise needs.  With a mask the tables come for the foreground
    and the background as well (``noise_table(which="bg")``: the noise away from structure).

    ``stats`` (a dict) receives ``seconds`` per phase (read, measure, download; the stream is synchronised around the
    phases only when ``stats`` is given), ``bricks``, ``passes`` (always 1), ``voxels_read`` -- per store, with the
    one-voxel halos -- and ``largest_alloc``, the most device bytes held here at one time (the readers' pools of
    decoded chunks are theirs and are not counted)."""
    from aind_exaspim_image_compression.utils import store_measure, store_windows
    budget = int(budget_bytes)
    if budget < 1:
        raise ValueError("budget_bytes must be positive")
    index = int(device) if device is not None else _native.default_device()
    arrs = store_windows.open_u16_stores("measure_store", (("src", src), ("mask", mask)), index)
    shape = tuple(int(s) for s in arrs[0].shape[2:])
    chunks = tuple(int(c) for c in arrs[0].chunks[2:])
    bricks = store_measure.plan_measure(shape, chunks, budget, mask is not None)
    ctx = _native.context(index)
    with store_windows.capped_pools(arrs, budget):
        return _measure(ctx, shape, bricks, store_windows.StoreWindows(arrs, chunks[0]), mask is not None, stats)


def measure_volume(vol, mask=None, device=None, stats=None):
    """``measure_store`` for a 3-D uint16 array in memory: uploaded whole and measured as one brick.  ``mask``: any
    array of the volume's shape, non-zero = foreground."""
    from aind_exaspim_image_compression.utils import store_compare, store_windows
    arrays = [np.asarray(vol)]
    if arrays[0].dtype != np.uint16 or arrays[0].ndim != 3 or 0 in arrays[0].shape:
        raise ValueError("measure_volume: vol is a 3-D uint16 array without an empty axis")
    if mask is not None:
        arrays.append((np.asarray(mask) != 0).astype(np.uint16))
        if arrays[1].shape != arrays[0].shape:
            raise ValueError("measure_volume: vol and mask must have one shape")
    shape = tuple(int(s) for s in arrays[0].shape)
    ctx = _native.context(device)
    brick = store_compare.Brick((0, 0, 0), shape, (0, 0, 0), shape, 2 * len(arrays) * int(np.prod(shape)))
    source = store_windows.ArrayWindows(ctx, [np.ascontiguousarray(a) for a in arrays])
    try:
        return _measure(ctx, shape, [brick], source, mask is not None, stats)
    finally:
        source.close()


def pg_params(noise):
    """``{"gain", "read_noise", "offset"}`` as floats from what the denoisers' ``noise=`` accepts: that dict (the
    return value of ``estimate_poisson_gaussian``) or an anscombe transform cfg (``anscombe_cfg``)."""
    if isinstance(noise, dict) and noise.get("kind") is not None:
        if noise["kind"] != "anscombe":
            raise ValueError("noise: a transform cfg must be of kind 'anscombe', not %r" % noise["kind"])
        noise = noise.get("params", {})
    if not isinstance(noise, dict):
        raise ValueError("noise must be a dict with gain, read_noise and offset, an anscombe cfg, or 'auto'")
    try:
        out = {k: float(noise[k]) for k in ("gain", "read_noise", "offset")}
    except KeyError as e:
        raise ValueError("noise: %s is missing" % e) from None
    if not (all(math.isfinite(v) for v in out.values()) and out["gain"] > 0.0 and out["read_noise"] >= 0.0):
        raise ValueError("noise: gain must be > 0, read_noise >= 0, all three finite (got %r)" % out)
    return out


def bound_table(noise, k, cap=65535):
    """uint16 [65536]: ``T[c] = min(cap, floor(k sqrt(gain max(c - offset, 0) + read_noise^2)))``, k noise standard
    deviations of a voxel of ``c`` counts under the Poisson-Gaussian model -- the table ``BlockBoundedCodec`` takes as
    its per-voxel error bound.  ``noise``: what ``pg_params`` accepts.  Host float64 throughout
    (IEEE products and square root), so the table is the same on every machine.  Host work only."""
    p = pg_params(noise)
    try:
        k = float(k)
    except (TypeError, ValueError):
        raise ValueError("bound_table: k must be a number") from None
    if not (math.isfinite(k) and k >= 0.0):
        raise ValueError("bound_table: k must be finite and >= 0 (got %r)" % k)
    cap = int(cap)
    if not 0 <= cap <= 65535:
        raise ValueError("bound_table: cap must be in [0, 65535]")
    c = np.arange(65536, dtype=np.float64)
    sigma = np.sqrt(p["gain"] * np.maximum(c - p["offset"], 0.0) + p["read_noise"] * p["read_noise"])
    return np.minimum(np.floor(k * sigma), float(cap)).astype(np.uint16)


def _stream(vol, dtype_in, dtype_out, device, run):
    arr = np.ascontiguousarray(vol, dtype=dtype_in)
    ctx = _native.context(device)
    d_in = ctx.to_device(arr.reshape(-1))
    d_out = ctx.alloc(max(1, arr.size) * np.dtype(dtype_out).itemsize)
    try:
        if arr.size:
            run(ctx, d_in, d_out, arr.size)
        ctx.sync()
        return d_out.download(arr.shape, dtype_out)
    finally:
        d_in.free()
        d_out.free()


def stabilise(vol, params, device=None):
    """The un-normalised generalised Anscombe transform of the uint16 counts ``vol`` as float32: noise of unit
    standard deviation under ``params``.  The forward stream of ``denoise_volume(noise=...)``."""
    nz = _native.pg_noise(**pg_params(params))
    return _stream(vol, np.uint16, np.float32, device, lambda ctx, a, b, n: ctx.gat_forward_u16(nz, a, b, n))


def unstabilise(D, params, inverse="closed_form", device=None):
    """uint16 counts from stabilised float32 values: the "closed_form" (exact unbiased, Makitalo & Foi),
    "asymptotic" (1/8) or "algebraic" (3/8) inverse, clipped to [0, 65535] and rounded half to even."""
    nz = _native.pg_noise(inverse=inverse, **pg_params(params))
    return _stream(D, np.float32, np.uint16, device, lambda ctx, a, b, n: ctx.gat_inverse_u16(nz, a, b, n))


def resolve_sigma(sigma, vol, device=None, **kw):
    """``sigma`` as a float; the string "auto" is measured from ``vol`` (see ``noise_table`` for what it may be)."""
    if isinstance(sigma, str):
        if sigma != "auto":
            raise ValueError("sigma must be a number or 'auto', not %r" % sigma)
        value = estimate_sigma(vol, device=device, **kw)
        if not (math.isfinite(value) and value > 0.0):
            raise ValueError("sigma='auto': the estimate is %r; the volume has no measurable noise" % value)
        return value
    return float(np.asarray(sigma).reshape(-1)[0])
