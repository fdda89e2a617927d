"""numpy restatements of the store-comparison operations, for the tests: the signed difference table,
the maximum projections, the samples an SSIM box reads, and the inputs the kernel tests share."""
import numpy as np

from util import synth_volume

DIFF_BINS = 131071


def box_slices(origin, dims):
    return tuple(slice(o, o + d) for o, d in zip(origin, dims))


def diff_table(ref, test, origin, dims, mask=None):
    """``hist[(test - ref) + 65535]`` over the box; with a mask ``(foreground, background)``."""
    sl = box_slices(origin, dims)
    d = test[sl].astype(np.int64) - ref[sl].astype(np.int64) + 65535
    if mask is None:
        return np.bincount(d.reshape(-1), minlength=DIFF_BINS).astype(np.uint64)
    fg = mask[sl] != 0
    return (np.bincount(d[fg], minlength=DIFF_BINS).astype(np.uint64),
            np.bincount(d[~fg], minlength=DIFF_BINS).astype(np.uint64))


def fold_mips(planes, ref, test, origin, dims):
    """Folds the box's maxima into ``planes``: ``{"ref" | "test" | "abs_diff": [yx, zx, zy]}`` of the volume's
    extents (``empty_mips``), in place."""
    sl = box_slices(origin, dims)
    r, t = ref[sl].astype(np.int64), test[sl].astype(np.int64)
    (z0, y0, x0), (dz, dy, dx) = origin, dims
    where = [(slice(y0, y0 + dy), slice(x0, x0 + dx)), (slice(z0, z0 + dz), slice(x0, x0 + dx)),
             (slice(z0, z0 + dz), slice(y0, y0 + dy))]
    for name, vol in (("ref", r), ("test", t), ("abs_diff", np.abs(t - r))):
        for axis in range(3):
            p = planes[name][axis]
            p[where[axis]] = np.maximum(p[where[axis]], vol.max(axis=axis).astype(np.uint16))
    return planes


def empty_mips(shape):
    nz, ny, nx = shape
    return {name: [np.zeros((ny, nx), np.uint16), np.zeros((nz, nx), np.uint16), np.zeros((nz, ny), np.uint16)]
            for name in ("ref", "test", "abs_diff")}


def whole_mips(ref, test):
    return fold_mips(empty_mips(ref.shape), ref, test, (0, 0, 0), ref.shape)


def reflect(i, n):
    """scipy.ndimage "reflect", by its definition: the axis mirrored about its edges, period 2 n."""
    period = list(range(n)) + list(range(n - 1, -1, -1))
    return period[i % (2 * n)]


def ssim_samples(b0, bd, n, window):
    """The set of indices in ``[0, n)`` the SSIM of the voxels ``[b0, b0 + bd)`` reads along one axis."""
    left = window // 2
    return {reflect(i, n) for i in range(b0 - left, b0 + bd + window - left - 1)}


def abs_percentile(ref, test, q):
    return float(np.percentile(np.abs(test.astype(np.int64) - ref.astype(np.int64)), q))


def mip_to_uint8(mip, low_pct=1.0, high_pct=99.9):
    m = np.asarray(mip, dtype=np.float32)
    lo = np.percentile(m, low_pct)
    hi = np.percentile(m, high_pct)
    span = hi - lo if hi > lo else 1.0
    return np.rint(np.clip((m - lo) / span, 0, 1) * 255).astype(np.uint8)


def renoised(vol, seed, sigma=9.0):
    """A second acquisition of ``vol``: the counts plus fresh noise, clipped and rounded."""
    rng = np.random.default_rng(seed)
    return np.rint(np.clip(vol.astype(np.float64) + rng.normal(0, sigma, vol.shape), 0, 65535)).astype(np.uint16)


def full_range_pair(shape, seed):
    """Counts over the whole range whose first elements are 0, 65535 against 65535, 0: both end bins."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 65536, shape).astype(np.uint16)
    b = rng.integers(0, 65536, shape).astype(np.uint16)
    a.reshape(-1)[:2] = [0, 65535]
    b.reshape(-1)[:2] = [65535, 0]
    return a, b


def synth_pair(shape, seed=0):
    vol, _ = synth_volume(shape, seed=seed, as_u16=True)
    return vol, renoised(vol, seed + 100)
