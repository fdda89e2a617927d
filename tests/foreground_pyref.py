"""Plain references for the foreground mask of a stored volume, numpy only: the cut that follows from
a table of the counts, and the mask of a box by the L1-ball definition.

Restated from the wording of include/exabm4d.h (``exabm4d_foreground_box_u16_dev``) and of
``StoreMeasure.foreground_threshold``; tests/test_store_foreground_host.py checks the restatement against
``mask_pyref`` (numpy's own median arithmetic, iterated cross dilation) without a GPU."""
import numpy as np


# ---- the threshold from the counts --------------------------------------------------------------------------------
def _median2(table):
    """Twice the median of the population ``table[i]`` times the value ``i``: the sum of the two middle values."""
    table = np.asarray(table).astype(object)              # Python integers: exact at any size
    n = int(table.sum())
    cum = np.cumsum(table)
    lo = int(np.searchsorted(cum, (n - 1) // 2 + 1))
    hi = int(np.searchsorted(cum, n // 2 + 1))
    return lo + hi


def threshold_from_counts(counts, k):
    """``mask_pyref.fg_threshold`` of any volume with these ``counts`` (65536 counters), as ``np.float32``.

    ``med`` is the mean of the two middle values: a multiple of 1/2 below 2^16, exact in fp32.  ``|v - med|`` is then
    exact too, and its median is half the median of ``|2 v - 2 med|``, whose table is the counts folded about
    ``2 med``; the mean of two such values is again a multiple of 1/4 below 2^17: exact.  What follows is numpy's
    arithmetic on an fp32 median with Python floats as weak scalars: ``1e-6``, ``1.4826`` and ``k`` are rounded to
    fp32, and each of the two additions and two multiplications rounds to fp32."""
    counts = np.asarray(counts)
    assert counts.shape == (65536,)
    med2 = _median2(counts)
    folded = np.zeros(2 * 65535 + 1, dtype=object)
    for v in np.nonzero(counts)[0]:
        folded[abs(2 * int(v) - med2)] += int(counts[v])
    mad4 = _median2(folded)                              # 4 mad = 2 (a + b) / 2 with a, b = |2 v - 2 med|
    f32 = np.float32
    med = f32(med2 / 2.0)
    mad = f32(mad4 / 4.0) + f32(1e-6)
    sigma = f32(1.4826) * mad
    with np.errstate(over="ignore"):
        return f32(med + f32(k) * sigma)


def cut_of_threshold(thr):
    """The least integer count above ``thr``, clamped to 0..65536 (65536: no count is)."""
    thr = float(thr)
    if thr < 0.0:
        return 0
    if thr >= 65535.0:
        return 65536
    return int(np.floor(thr)) + 1


def cut_from_counts(counts, k):
    return cut_of_threshold(threshold_from_counts(counts, k))


# ---- the mask of a box ------------------------------------------------------------------------------------------------
def ball_dilate(seeds, radius):
    """Dilation of the (z, y, x) boolean array ``seeds`` by the L1 ball of ``radius``, cut at the array's faces: the OR
    of the array shifted by every offset with |dz| + |dy| + |dx| <= radius, zeros shifted in."""
    seeds = np.asarray(seeds, dtype=bool)
    out = np.zeros_like(seeds)
    nz, ny, nx = seeds.shape
    r = int(radius)
    for dz in range(-r, r + 1):
        for dy in range(-(r - abs(dz)), r - abs(dz) + 1):
            rest = r - abs(dz) - abs(dy)
            for dx in range(-rest, rest + 1):
                src = tuple(slice(max(0, -d), max(0, n - max(0, d))) for d, n in zip((dz, dy, dx), (nz, ny, nx)))
                dst = tuple(slice(max(0, d), max(0, d) + (s.stop - s.start)) for d, s in zip((dz, dy, dx), src))
                if all(s.stop > s.start for s in src):
                    out[dst] |= seeds[src]
    return out


def box_mask(vol, cut, radius, box_origin, box_dims, value=1):
    """``exabm4d_foreground_box_u16_dev``'s out_u16 for the box: ``value`` where a voxel of ``vol`` with a count
    ``>= cut`` lies within the L1 distance ``radius``, computed from the box grown by ``radius`` and cut at the
    volume's faces only.  Also returns (seeds in the box, mask voxels in the box)."""
    vol = np.asarray(vol)
    r = int(radius)
    lo = [max(0, o - r) for o in box_origin]
    hi = [min(n, o + d + r) for o, d, n in zip(box_origin, box_dims, vol.shape)]
    seeds = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.int64) >= int(cut)
    inner = tuple(slice(o - l, o - l + d) for o, l, d in zip(box_origin, lo, box_dims))
    mask = ball_dilate(seeds, r)[inner]
    return (mask * int(value)).astype(np.uint16), (int(seeds[inner].sum()), int(mask.sum()))
