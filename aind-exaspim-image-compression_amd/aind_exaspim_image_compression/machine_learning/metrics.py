"""Count-space quality metrics, reduced on the GPU.

Drop-in for the scoring half of the reference's ``machine_learning/metrics.py`` (lines 306-450):
``foreground_background_mae``, ``mip_max_error``, ``false_bright_rate``, ``evaluate_example``,
``checkpoint_score`` with the reference's signatures and return values.  The reference makes
float64 copies of every image and reduces them with numpy; here each image is uploaded once (or
is already a device buffer), one HIP kernel accumulates the masked absolute-error sums, maxima
and the bright-voxel count (``exabm4d_masked_error_stats_dev``), and the percentiles / median /
MAD come from device histograms (``utils/order_stats.py``).  Integer-valued inputs give the
reference's numbers exactly; float inputs differ only by fp64 summation order.

The mask builders and the coherence gate of the reference module (lines 32-303) are here too,
with the reference's names, signatures, defaults and return types: ``make_foreground_mask``,
``local_autocorr``, ``highfreq_energy_fraction``, ``make_segmentation_mask``,
``patch_has_incoherent_segment`` and ``make_skeleton_mask``; plus the batched forms
``foreground_masks`` and ``incoherent_segments`` that take (B, z, y, x) arrays and make one device
pass each.  The per-patch median / MAD threshold, the binary dilation, the Gaussian
smoothing (scipy's ``gaussian_filter`` bit for bit), the distinct-label set and the per-segment
two-pass statistics are HIP kernels (``csrc/mask_kernels.hip``); the host only rasterises skeleton
points, sorts the short label lists and applies the reference's finishing rules to the sums.
``evaluate_examples`` is ``evaluate_example`` of every example of a (B, z, y, x) batch in one device pass
(``exabm4d_evaluate_batch_dev``): what ``train.validate`` scores a validation set with.
There is no CPU fallback: without a GPU they raise ``NativeError``.
"""
import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import order_stats
from aind_exaspim_image_compression.utils.store_foreground import (  # noqa: F401
    _check_filter_args, foreground_store, foreground_volume)
from aind_exaspim_image_compression.utils.store_segment import components_store, components_volume  # noqa: F401

# reference metrics.py:24-29
DEFAULT_CHECKPOINT_WEIGHTS = {
    "fg_mae": 1.0,
    "bg_mae": 0.2,
    "top_pct_error": 0.5,
    "cratio": 0.0,
}


class DeviceImage:
    """An image in HBM with the element type the kernels read (uint16, float32 or float64).

    uint16 and float32 arrays are uploaded as they are; every other dtype is widened to float64,
    which is what the reference converts everything to."""

    def __init__(self, arr, ctx=None):
        arr = np.asarray(arr)
        self.orig_dtype = arr.dtype
        if arr.dtype == np.bool_:
            arr = arr.astype(np.uint16)
        if arr.dtype not in (np.uint16, np.float32, np.float64):
            arr = arr.astype(np.float64)
        self.ctx = ctx or _native.context()
        self.shape = arr.shape
        self.dtype = arr.dtype
        self.n = int(arr.size)
        if self.n == 0:
            raise ValueError("empty image")
        self.buf = self.ctx.to_device(np.ascontiguousarray(arr).reshape(-1))
        self._stats = None

    def free(self):
        self.buf.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def order_stats(self):
        """Exact order statistics of the image as float64 values."""
        if self._stats is None:
            if self.dtype == np.uint16:
                hist = self.ctx.u16_histogram(self.buf, self.n)
                self._stats = order_stats.from_u16_hist(hist, dtype=np.float64)
            else:
                self._stats = order_stats.DeviceOrderStats(self.ctx, self.buf, self.dtype, self.n)
        return self._stats

    def median_abs_deviation(self, center):
        """``np.median(np.abs(x - center))`` of the float64-widened image."""
        if self.dtype == np.uint16:
            return order_stats.median_abs_deviation(self.order_stats(), center)
        dev = order_stats.DeviceOrderStats(self.ctx, self.buf, self.dtype, self.n,
                                           center=float(center))
        return order_stats.median(dev)


def _mask_buffer(ctx, fg_mask, n):
    fg = np.ascontiguousarray(np.asarray(fg_mask, dtype=bool)).reshape(-1)
    if fg.size != n:
        raise ValueError("mask and image sizes differ")
    return ctx.to_device(fg.view(np.uint8))


def _stats(pred, ref, mask_buf, thr=float("inf")):
    if pred.n != ref.n:
        raise ValueError("images must have the same number of voxels")
    return pred.ctx.masked_error_stats(pred.buf, pred.dtype, ref.buf, ref.dtype, mask_buf, pred.n,
                                       thr)


def _split_mae(out, n):
    n_fg = int(out[2])
    n_bg = n - n_fg
    fg_mae = float(out[0] / n_fg) if n_fg else 0.0
    bg_mae = float(out[1] / n_bg) if n_bg else 0.0
    return fg_mae, bg_mae


def foreground_background_mae(pred, ref, fg_mask):
    """(foreground MAE, background MAE) of ``pred`` against ``ref`` (reference metrics.py:306-330);
    a side with no voxels reports 0."""
    with DeviceImage(pred) as p, DeviceImage(ref, p.ctx) as r:
        m = _mask_buffer(p.ctx, fg_mask, p.n)
        try:
            return _split_mae(_stats(p, r, m), p.n)
        finally:
            m.free()


def _mip_error(out, pred, raw):
    """``float(abs(np.max(pred) - np.max(raw)))`` with numpy's scalar arithmetic of the callers'
    dtypes -- including the reference's wrap-around when both are uint16 and the prediction's
    maximum is the smaller one (metrics.py:349 subtracts two uint16 scalars)."""
    pm, rm = np.float64(out[4]), np.float64(out[5])
    if pred.orig_dtype.kind in "iu":
        pm = pred.orig_dtype.type(pm)
    if raw.orig_dtype.kind in "iu":
        rm = raw.orig_dtype.type(rm)
    if pred.orig_dtype == np.float32:
        pm = np.float32(pm)
    if raw.orig_dtype == np.float32:
        rm = np.float32(rm)
    with np.errstate(over="ignore"):
        return float(abs(pm - rm))


def mip_max_error(pred, raw):
    """|max(pred) - max(raw)| (reference metrics.py:333-349)."""
    with DeviceImage(pred) as p, DeviceImage(raw, p.ctx) as r:
        return _mip_error(_stats(p, r, None), p, r)


def _bright_threshold(raw, k):
    med = order_stats.median(raw.order_stats())
    mad = raw.median_abs_deviation(med) + 1e-6
    return med + k * 1.4826 * mad


def false_bright_rate(pred, raw, fg_mask, k=6.0):
    """Fraction of background voxels where ``pred`` exceeds median(raw) + k * 1.4826 * MAD(raw)
    (reference metrics.py:352-381)."""
    with DeviceImage(pred) as p, DeviceImage(raw, p.ctx) as r:
        m = _mask_buffer(p.ctx, fg_mask, p.n)
        try:
            out = _stats(p, r, m, float("inf"))
            n_bg = p.n - int(out[2])
            if not n_bg:
                return 0.0
            thr = _bright_threshold(r, k)
            out = _stats(p, r, m, float(thr))
            return float(out[3] / n_bg)
        finally:
            m.free()


def evaluate_example(pred, raw, target, fg_mask, pct=0.1):
    """The metric dictionary of one example, in counts (reference metrics.py:384-424): foreground
    fidelity against ``raw``, background cleanup against the BM4D ``target``, bright-tail
    percentile error / preservation, MIP maximum error and the false-bright rate."""
    with DeviceImage(pred) as p, DeviceImage(raw, p.ctx) as r, DeviceImage(target, p.ctx) as t:
        m = _mask_buffer(p.ctx, fg_mask, p.n)
        try:
            n_bg = p.n - int(_stats(p, r, m)[2])
            thr = _bright_threshold(r, 6.0) if n_bg else float("inf")
            vs_raw = _stats(p, r, m, float(thr))
            vs_target = _stats(p, t, m)
        finally:
            m.free()
        fg_mae, _ = _split_mae(vs_raw, p.n)
        _, bg_mae = _split_mae(vs_target, p.n)
        q = 100.0 - pct
        raw_top = float(order_stats.percentile(r.order_stats(), q))
        pred_top = float(order_stats.percentile(p.order_stats(), q))
        # np.percentile of a sample that holds a NaN is NaN (the radix selection would rank it as an extreme);
        # the maxima say whether one is there
        if np.isnan(vs_raw[4]):
            pred_top = float("nan")
        if np.isnan(vs_raw[5]):
            raw_top = float("nan")
        return {
            "fg_mae": fg_mae,
            "bg_mae": bg_mae,
            "top_pct_error": abs(pred_top - raw_top),
            "top_pct_preservation": pred_top / (raw_top + 1e-8),
            "mip_max_error": _mip_error(vs_raw, p, r),
            "false_bright_rate": float(vs_raw[3] / n_bg) if n_bg else 0.0,
        }


# ---- a batch of examples in one device pass ---------------------------------------
class _AskedRanks:
    """Stands in for a sample of ``n`` values and records the ranks ``order_stats.percentile`` reads,
    so the ranks the kernel selects are the ones that code interpolates between."""

    def __init__(self, n):
        self.n, self.asked = n, []

    def at(self, k):
        self.asked.append(k + self.n if k < 0 else k)
        return np.float64(0.0)


class _RankValues:
    """The values the kernel selected at those ranks, for ``order_stats.percentile(..., at=...)``."""

    def __init__(self, n, ranks, values):
        self.n = n
        self.values = {int(r): np.float64(v) for r, v in zip(ranks, values)}
        self.any = np.float64(values[0])

    def at(self, k):
        return self.values.get(k + self.n if k < 0 else k, self.any)    # any value answers the dtype probe


class _OrigDtype:
    def __init__(self, dtype):
        self.orig_dtype = np.dtype(dtype)


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _torch_np_dtype(t):
    import torch
    table = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16,
             torch.uint8: np.uint8, torch.bool: np.bool_, torch.int16: np.int16, torch.int32: np.int32}
    if hasattr(torch, "uint16"):
        table[torch.uint16] = np.uint16
    return np.dtype(table.get(t.dtype, np.void))


def _example_images(arrays, names):
    """(B, z, y, x) uint16 / float32 operands, all numpy arrays or all CUDA tensors of one shape."""
    on_device = [_is_device_tensor(a) for a in arrays]
    if any(on_device) and not all(on_device):
        raise ValueError("pred, raw, target and fg_mask must all be host arrays or all be CUDA tensors")
    if not on_device[0]:
        arrays = [np.asarray(a) for a in arrays]
    shape = tuple(int(s) for s in arrays[0].shape)
    if len(shape) != 4:
        raise ValueError(f"{names[0]} must be (B, z, y, x), got shape {shape}")
    for a, name in zip(arrays, names):
        if tuple(int(s) for s in a.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(a.shape)}, {names[0]} has {shape}")
    dtypes = [_torch_np_dtype(a) if on_device[0] else a.dtype for a in arrays]
    for dt, name in zip(dtypes[:3], names):
        if dt not in (np.uint16, np.float32):
            raise ValueError(f"{name} must be uint16 or float32, not {dt}")
    if dtypes[3].kind not in "buf" or (dtypes[3].kind == "u" and dtypes[3] != np.uint8):
        raise ValueError(f"fg_mask must be bool, uint8 or float, not {dtypes[3]}")
    return arrays, dtypes, shape, on_device[0]


def evaluate_examples(pred, raw, target, fg_mask, pct=0.1):
    """``evaluate_example`` of every example of a batch: a list of B dicts with its keys and values.

    ``pred`` / ``raw`` / ``target``: (B, z, y, x) uint16 or float32, each its own type; ``fg_mask``: bool, uint8
    (non-zero = foreground) or float (``> 0.5``).  All four are numpy arrays (one upload each) or CUDA tensors
    of one device (read in place on torch's current stream).  One device pass and one synchronisation for the
    whole batch (``Context.evaluate_batch``): medians, MAD, threshold and the percentile neighbours are
    selected per patch inside the kernel; the host finishes each row with the arithmetic ``evaluate_example``
    uses."""
    arrays, dtypes, shape, on_device = _example_images([pred, raw, target, fg_mask],
                                                       ["pred", "raw", "target", "fg_mask"])
    batch, n = shape[0], shape[1] * shape[2] * shape[3]
    if batch == 0:
        return []
    if n == 0:
        raise ValueError("empty image")
    q = 100.0 - pct
    asked = _AskedRanks(n)
    order_stats.percentile(asked, q, at=asked.at)        # raises for a pct outside [0, 100]
    pct_ranks = sorted(asked.asked[-2:])
    ranks = [(n - 1) // 2, n // 2] + pct_ranks
    p, r, t, m = arrays
    if on_device:
        import torch
        dev = p.device
        if any(a.device != dev for a in arrays):
            raise ValueError("pred, raw, target and fg_mask must be on one device")
        m = (m > 0.5) if dtypes[3].kind == "f" else m
        ops = [a.contiguous() for a in (p, r, t, m)]
        ctx = _native.context(dev.index or 0)
        with torch.cuda.device(dev):
            ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            try:
                rows = ctx.evaluate_batch(ops[0], dtypes[0], ops[1], dtypes[1], ops[2], dtypes[2], ops[3],
                                          batch, n, 6.0, ranks)
            finally:
                ctx.reset_stream()
    else:
        m = (m > 0.5) if dtypes[3].kind == "f" else m
        ctx = _native.context()
        bufs = []
        try:
            for a in (p, r, t, np.ascontiguousarray(m).view(np.uint8)):
                bufs.append(ctx.to_device(np.ascontiguousarray(a).reshape(-1)))
            rows = ctx.evaluate_batch(bufs[0], dtypes[0], bufs[1], dtypes[1], bufs[2], dtypes[2], bufs[3], batch,
                                      n, 6.0, ranks)
        finally:
            for b in bufs:
                b.free()
    p_dt, r_dt = _OrigDtype(dtypes[0]), _OrigDtype(dtypes[1])
    out = []
    for row in rows:
        fg_mae, bg_mae = _split_mae(row, n)
        n_bg = n - int(row[2])
        tops = []
        for lo in (_native.EVAL_RAW_LO, _native.EVAL_PRED_LO):
            picked = _RankValues(n, pct_ranks, row[lo:lo + 2])
            with np.errstate(invalid="ignore"):         # inf - inf between two infinite neighbours: NaN, as in numpy
                tops.append(float(order_stats.percentile(picked, q, at=picked.at)))
        raw_top, pred_top = tops
        out.append({
            "fg_mae": fg_mae,
            "bg_mae": bg_mae,
            "top_pct_error": abs(pred_top - raw_top),
            "top_pct_preservation": pred_top / (raw_top + 1e-8),
            "mip_max_error": _mip_error(row, p_dt, r_dt),
            "false_bright_rate": float(row[3] / n_bg) if n_bg else 0.0,
        })
    return out


def checkpoint_score(metrics, cratio, weights=None):
    """Checkpoint-selection score, lower is better (reference metrics.py:427-450)."""
    w = DEFAULT_CHECKPOINT_WEIGHTS if weights is None else weights
    return (
        w.get("fg_mae", 0.0) * metrics["fg_mae"]
        + w.get("bg_mae", 0.0) * metrics["bg_mae"]
        + w.get("top_pct_error", 0.0) * metrics["top_pct_error"]
        - w.get("cratio", 0.0) * cratio
    )


# ---- patch-cache mask builders and coherence gate (reference metrics.py:32-303) -----------------
GAUSS_TRUNCATE = 4.0        # scipy.ndimage.gaussian_filter's default truncate
_SEG = {"n": 0, "mean_raw": 1, "mean_hf": 2, "ss_raw": 3, "ss_hf": 4, "axes": 5}   # segment_stats columns


def gaussian_weights(sigma):
    """The centre-and-right half of scipy's ``_gaussian_kernel1d(sigma, 0, int(4 * sigma + 0.5))``,
    computed the way scipy computes it (the kernel is symmetric bit for bit).  A sigma scipy skips
    (<= 1e-15) gives the identity kernel."""
    if float(sigma) <= 1e-15:
        return np.ones(1, dtype=np.float64)
    radius = int(GAUSS_TRUNCATE * float(sigma) + 0.5)
    if radius > _native.GAUSS_MAX_RADIUS:
        raise ValueError(f"smooth_sigma {sigma} needs a radius above {_native.GAUSS_MAX_RADIUS}")
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x[radius:])


def autocorr_from_stats(st):
    """``local_autocorr`` from one row of segment statistics (``SEG_STATS_K`` columns): the
    reference's rules (metrics.py:100-113) on centred pair sums."""
    vals = []
    for ax in range(3):
        n, _, _, sxx, syy, sxy = (float(v) for v in st[_SEG["axes"] + 6 * ax:_SEG["axes"] + 6 * ax + 6])
        if n < 2:
            continue
        if np.sqrt(sxx / n) < 1e-6 or np.sqrt(syy / n) < 1e-6:
            continue
        # np.corrcoef: cov / stddev / stddev, clipped to [-1, 1]
        c = (sxy / (n - 1)) / np.sqrt(sxx / (n - 1)) / np.sqrt(syy / (n - 1))
        vals.append(float(np.clip(c, -1.0, 1.0)))
    return float(np.mean(vals)) if vals else 1.0


def highfreq_from_stats(st):
    """``highfreq_energy_fraction`` from one row of segment statistics (metrics.py:150-155):
    0.0 when the masked variance is below 1e-12, NaN for an empty mask (numpy's var of nothing)."""
    n = float(st[_SEG["n"]])
    if n == 0:
        return float("nan")
    var_v = float(st[_SEG["ss_raw"]]) / n
    if var_v < 1e-12:
        return 0.0
    return float((float(st[_SEG["ss_hf"]]) / n) / var_v)


def _patches(arr, ndim, name):
    arr = np.asarray(arr)
    if arr.ndim != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {arr.shape}")
    if 0 in arr.shape[-3:]:
        raise ValueError(f"{name} has an empty axis: {arr.shape}")
    return arr


def _raw_f32(raw):
    """uint16 converts to float32 exactly on the device; everything else is cast on the host, as
    the reference casts it (``np.asarray(raw, dtype=np.float32)``)."""
    return np.ascontiguousarray(raw if raw.dtype == np.uint16 else raw.astype(np.float32, copy=False))


def _raw_f64(raw):
    """The reference widens raw to float64; uint16 and float32 widen exactly on the device."""
    if raw.dtype in (np.uint16, np.float32):
        return np.ascontiguousarray(raw.astype(np.float32, copy=False))
    return np.ascontiguousarray(raw.astype(np.float64, copy=False))


def _labels_dev(labels):
    """Labels as an element type the device reads: uint8 / uint32 / uint64 / int32 / int64."""
    if labels.dtype == np.bool_:
        return np.ascontiguousarray(labels.view(np.uint8))
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers, got {labels.dtype}")
    if labels.dtype in (np.uint8, np.uint32, np.uint64, np.int32, np.int64):
        return np.ascontiguousarray(labels)
    return np.ascontiguousarray(labels.astype(np.uint32 if labels.dtype.kind == "u" else np.int32))


def foreground_masks(raw, k=6.0, dilate=1):
    """``make_foreground_mask`` of every patch of ``raw`` (B, z, y, x) in one device pass:
    a (B, z, y, x) bool array."""
    raw = _patches(raw, 4, "raw")
    if raw.shape[0] == 0:
        return np.zeros(raw.shape, dtype=bool)
    src = _raw_f32(raw)
    ctx = _native.context()
    with ctx.to_device(src) as d_raw, ctx.alloc(src.size) as d_mask:
        ctx.foreground_masks(d_raw, src.dtype, src.shape[0], src.shape[1:], k, max(int(dilate), 0), d_mask)
        return d_mask.download(src.shape, np.uint8).view(bool)


def _dilate(masks, iterations):
    """scipy.ndimage.binary_dilation(m, iterations) of every (z, y, x) mask of ``masks`` (B, ...)."""
    m = np.ascontiguousarray(masks, dtype=bool).view(np.uint8)
    ctx = _native.context()
    with ctx.to_device(m) as d_in, ctx.alloc(m.size) as d_out:
        ctx.binary_dilate(d_in, m.shape[0], m.shape[1:], max(int(iterations), 0), d_out)
        return d_out.download(m.shape, np.uint8).view(bool)


def _binary_volume(who, mask):
    mask = np.asarray(mask)
    if mask.ndim != 3 or 0 in mask.shape or mask.size >= 2 ** 31:
        raise ValueError("%s: mask is a 3-D array without an empty axis and with fewer than 2^31 voxels" % who)
    return np.ascontiguousarray(mask != 0).view(np.uint8)


def label_components(mask, connectivity=26, relabel=False):
    """The connected components of the non-zero voxels of a 3-D ``mask`` on the device:
    ``(labels, n)``, int32 labels and the number of components.  A component's label is 1 + the linear (z, y, x)
    index of its first voxel in raster order, background 0; ``relabel=True`` renumbers them 1..n in that order on the
    host, which is ``scipy.ndimage.label``'s numbering.  ``connectivity``: 6 (faces) or 26 (faces, edges, corners)."""
    _check_filter_args("label_components", 1, connectivity)
    m = _binary_volume("label_components", mask)
    ctx = _native.context()
    with ctx.to_device(m) as d_mask, ctx.alloc(4 * m.size) as d_labels, ctx.alloc(24) as d_counts:
        # no component has 2^31 - 1 voxels unless it is the whole array: every one counts as dropped, or one as kept
        ctx.label_components(d_mask, np.uint8, m.shape, min_voxels=2 ** 31 - 1, connectivity=connectivity,
                             labels=d_labels, counts=d_counts)
        labels = d_labels.download(m.shape, np.uint32).view(np.int32)
        _, kept, dropped = (int(c) for c in d_counts.download((3,), np.uint64))
    n = dropped + (1 if kept else 0)
    if relabel and n:
        flat = labels.reshape(-1)
        firsts = np.flatnonzero(flat == np.arange(1, flat.size + 1, dtype=np.int64))     # roots, in raster order
        table = np.zeros(flat.size + 1, dtype=np.int32)
        table[firsts + 1] = np.arange(1, firsts.size + 1, dtype=np.int32)
        labels = table[flat].reshape(labels.shape)
    return labels, n


def remove_small_components(mask, min_voxels, connectivity=26):
    """``mask`` (3-D) without the connected components of fewer than ``min_voxels`` voxels, as a bool array, on the
    device.  The array is resident and the sizes are the whole array's, so ``min_voxels`` is any integer >= 1."""
    min_voxels = _check_filter_args("remove_small_components", min_voxels, connectivity, least=1)
    m = _binary_volume("remove_small_components", mask)
    ctx = _native.context()
    with ctx.to_device(m) as d_mask, ctx.alloc(m.size) as d_kept:
        ctx.label_components(d_mask, np.uint8, m.shape, min_voxels=min_voxels, connectivity=connectivity,
                             kept_u8=d_kept)
        return d_kept.download(m.shape, np.uint8).view(bool)


def make_foreground_mask(raw, k=6.0, dilate=1, min_voxels=0, connectivity=26):
    """Robust intensity foreground mask, raw > median + k * 1.4826 * MAD, then ``dilate`` binary
    dilations (reference metrics.py:32-62): ``foreground_masks`` with B = 1.  With ``min_voxels`` > 0 the voxels above
    the threshold are filtered first: only connected components (``connectivity`` 6 or 26) of at least ``min_voxels``
    voxels are dilated (threshold, filter, dilate)."""
    min_voxels = _check_filter_args("make_foreground_mask", min_voxels, connectivity)
    raw = _patches(raw, 3, "raw")
    if min_voxels == 0:
        return foreground_masks(raw[None], k, dilate)[0]
    seeds = remove_small_components(foreground_masks(raw[None], k, 0)[0], min_voxels, connectivity)
    return _dilate(seeds[None], dilate)[0]


def make_segmentation_mask(labels, dilate=0):
    """``labels > 0``, dilated ``dilate`` times on the device (reference metrics.py:161-199)."""
    labels = _patches(labels, 3, "labels")
    return _dilate((labels > 0)[None], dilate if dilate > 0 else 0)[0]


def make_skeleton_mask(points, start, patch_shape, dilate=2):
    """Skeleton points inside the patch rasterised as the reference does, then ``dilate`` binary
    dilations on the device (reference metrics.py:263-303)."""
    start = np.asarray(start)
    stop = start + np.asarray(patch_shape)
    pts = np.asarray(points)
    inside = np.all((pts >= start) & (pts < stop), axis=1)
    mask = np.zeros(tuple(patch_shape), dtype=bool)
    local = (pts[inside] - start).astype(int)
    if local.size:
        mask[local[:, 0], local[:, 1], local[:, 2]] = True
    mask = _patches(mask, 3, "patch")
    return _dilate(mask[None], dilate if dilate > 0 else 0)[0]


def _segment_stats(ctx, d_labels, label_dtype, d_raw, raw_dtype, d_smooth, batch, shape, lag,
                   item_patch, item_key):
    lag = int(lag)
    if lag < 1:
        raise ValueError("lag must be >= 1")
    return ctx.segment_stats(d_labels, label_dtype, d_raw, raw_dtype, d_smooth, batch, shape, lag,
                             item_patch, item_key)


def _single_mask_stats(raw, mask, lag, smooth, smooth_sigma):
    """Segment statistics of one boolean mask over one patch (the mask is label 1)."""
    raw = _patches(raw, 3, "raw")
    mask = np.asarray(mask, dtype=bool)
    if mask.shape != raw.shape:
        raise ValueError("raw and mask shapes differ")
    src = _raw_f64(raw)
    m = np.ascontiguousarray(mask).view(np.uint8)
    ctx = _native.context()
    with ctx.to_device(src) as d_raw, ctx.to_device(m) as d_mask:
        d_smooth = None
        try:
            if smooth is not None:
                sm = np.asarray(smooth, dtype=np.float64)
                if sm.shape != raw.shape:
                    raise ValueError("raw and smooth shapes differ")
                d_smooth = ctx.to_device(sm)
            elif smooth_sigma is not None:
                d_smooth = ctx.alloc(src.size * 8)
                ctx.gaussian_filter3d(d_raw, src.dtype, 1, src.shape, gaussian_weights(smooth_sigma), d_smooth)
            return _segment_stats(ctx, d_mask, np.uint8, d_raw, src.dtype, d_smooth, 1, src.shape, lag,
                                  [0], [1])[0]
        finally:
            if d_smooth is not None:
                d_smooth.free()


def local_autocorr(raw, mask, lag=2):
    """Mean over the axes of the Pearson correlation of masked voxel pairs ``lag`` apart; 1.0 when
    no axis can be measured (reference metrics.py:65-113)."""
    return autocorr_from_stats(_single_mask_stats(raw, mask, lag, None, None))


def highfreq_energy_fraction(raw, mask, smooth=None, smooth_sigma=1.0):
    """``var(raw - smooth) / var(raw)`` over the mask, ``smooth`` the Gaussian-smoothed raw
    (computed on the device when not given); 0.0 when the masked variance is below 1e-12
    (reference metrics.py:116-158)."""
    return highfreq_from_stats(_single_mask_stats(raw, mask, 1, smooth, smooth_sigma))


def _label_lists(ctx, d_labels, labels, batch, shape):
    """Per patch, np.unique(labels[labels > 0], return_counts=True): the device set, sorted here;
    a patch the set cannot hold is counted on the host."""
    keys, counts, held, status = ctx.label_set(d_labels, labels.dtype, batch, shape)
    out = []
    for b in range(batch):
        if status[b]:
            lb = labels[b]
            u, c = np.unique(lb[lb > 0], return_counts=True)
            out.append((u.astype(np.uint64), c.astype(np.int64)))
        else:
            k = keys[b, :held[b]]
            order = np.argsort(k, kind="stable")
            out.append((k[order], counts[b, :held[b]][order].astype(np.int64)))
    return out


def segment_scores(labels, raw, min_segment_voxels=50, smooth_sigma=1.0, coherence_lag=2):
    """For every patch of (B, z, y, x) ``labels`` / ``raw``, the list of
    ``(label, voxels, autocorr, highfreq)`` of its segments with at least ``min_segment_voxels``
    voxels, in ``np.unique`` order: what ``patch_has_incoherent_segment`` decides on."""
    labels = _patches(labels, 4, "labels")
    raw = _patches(raw, 4, "raw")
    if labels.shape != raw.shape:
        raise ValueError("labels and raw shapes differ")
    batch, shape = labels.shape[0], labels.shape[1:]
    scores = [[] for _ in range(batch)]
    if batch == 0:
        return scores
    lab = _labels_dev(labels)
    ctx = _native.context()
    with ctx.to_device(lab) as d_labels:
        lists = _label_lists(ctx, d_labels, lab, batch, shape)
        item_patch, item_key, item_count = [], [], []
        for b, (keys, counts) in enumerate(lists):
            keep = counts >= min_segment_voxels
            item_patch += [b] * int(keep.sum())
            item_key += [int(x) for x in keys[keep]]
            item_count += [int(x) for x in counts[keep]]
        if not item_patch:
            return scores
        src = _raw_f64(raw)
        with ctx.to_device(src) as d_raw, ctx.alloc(src.size * 8) as d_smooth:
            ctx.gaussian_filter3d(d_raw, src.dtype, batch, shape, gaussian_weights(smooth_sigma), d_smooth)
            st = _segment_stats(ctx, d_labels, lab.dtype, d_raw, src.dtype, d_smooth, batch, shape,
                                coherence_lag, item_patch, np.array(item_key, dtype=np.uint64))
    for b, key, cnt, row in zip(item_patch, item_key, item_count, st):
        scores[b].append((key, cnt, autocorr_from_stats(row), highfreq_from_stats(row)))
    return scores


def incoherent_segments(labels, raw, min_autocorr=0.4, max_highfreq_frac=0.35, min_segment_voxels=50,
                        smooth_sigma=1.0, coherence_lag=2):
    """``patch_has_incoherent_segment`` of every patch of (B, z, y, x) ``labels`` / ``raw`` in one
    device pass: a (B,) bool array."""
    scores = segment_scores(labels, raw, min_segment_voxels, smooth_sigma, coherence_lag)
    return np.array([any(not (ac >= min_autocorr) and hf > max_highfreq_frac for _, _, ac, hf in seg)
                     for seg in scores], dtype=bool)


def patch_has_incoherent_segment(labels, raw, min_autocorr=0.4, max_highfreq_frac=0.35,
                                 min_segment_voxels=50, smooth_sigma=1.0, coherence_lag=2):
    """True when a segment of at least ``min_segment_voxels`` voxels fails both coherence tests:
    lag-``coherence_lag`` autocorrelation below ``min_autocorr`` and high-frequency energy fraction
    above ``max_highfreq_frac`` (reference metrics.py:202-260): ``incoherent_segments`` with B = 1."""
    labels = _patches(labels, 3, "labels")
    raw = _patches(raw, 3, "raw")
    return bool(incoherent_segments(labels[None], raw[None], min_autocorr, max_highfreq_frac,
                                    min_segment_voxels, smooth_sigma, coherence_lag)[0])
