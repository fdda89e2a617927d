"""Plain references for csrc/mask_kernels.hip, numpy and the standard library only (the GPU machine may
lack scipy): the foreground threshold and mask, binary dilation, the fp64 Gaussian, the label counts, the
23 segment-statistics columns in exact rational arithmetic, and the error bound of the float columns.

Restated from the wording of include/exabm4d.h and from numpy / scipy semantics; tests/test_mask_pyref.py
checks the restatement against scipy and the committed fixture without a GPU."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SEG_STATS_K = 23


# ---- foreground threshold and mask -------------------------------------------------------------------------
def fg_threshold(raw, k):
    """make_foreground_mask's threshold, every step in numpy's fp32 arithmetic (``k`` a Python float, which
    numpy rounds to fp32).  A NaN in ``raw`` makes the median NaN; an infinite median makes |raw - med| hold
    a NaN: in both cases the threshold is NaN, exactly as numpy gives it."""
    raw = np.asarray(raw, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        med = np.median(raw)
        mad = np.median(np.abs(raw - med)) + 1e-6
        sigma = 1.4826 * mad
        return np.float32(med + float(k) * sigma)


def fg_mask(raw, k, dilate_iterations):
    raw = np.asarray(raw, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        mask = raw > fg_threshold(raw, k)          # nothing is above a NaN threshold
    return dilate(mask, dilate_iterations)


# ---- binary dilation -------------------------------------------------------------------------------------
def dilate(mask, iterations):
    """``iterations`` passes of the 6-neighbour cross over a (z, y, x) mask, border 0: six shifted ORs."""
    m = np.asarray(mask) != 0
    for _ in range(int(iterations)):
        out = m.copy()
        for ax in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            out[tuple(hi)] |= m[tuple(lo)]
            out[tuple(lo)] |= m[tuple(hi)]
        m = out
    return m


# ---- Gaussian ----------------------------------------------------------------------------------------------
def reflect(i, n):
    """Index of scipy's "reflect" boundary (d c b a | a b c d | d c b a), period 2n, any distance outside."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian(x, weights):
    """exabm4d_gaussian_filter3d_dev as the header states it: axes 0, 1, 2 in turn in float64; per output
    acc = x[0] w[0], then acc += (x[-j] + x[+j]) w[j] for j = radius .. 1, indices reflected with period 2n.
    ``weights`` is the centre-and-right half of the kernel."""
    w = np.asarray(weights, dtype=np.float64)
    out = np.asarray(x).astype(np.float64)
    for ax in range(3):
        n = out.shape[ax]
        idx = np.arange(n)
        acc = out * w[0]
        for j in range(len(w) - 1, 0, -1):
            pair = np.take(out, reflect(idx - j, n), axis=ax) + np.take(out, reflect(idx + j, n), axis=ax)
            acc += pair * w[j]
        out = acc
    return out


# ---- labels --------------------------------------------------------------------------------------------------
def label_counts(labels):
    labels = np.asarray(labels)
    return np.unique(labels[labels > 0], return_counts=True)


def segment_mask(labels, key):
    """Voxels whose label equals ``key``; labels <= 0 and key 0 never form a segment."""
    labels = np.asarray(labels)
    key = int(key)
    if key <= 0 or key > int(np.iinfo(labels.dtype).max):
        return np.zeros(labels.shape, dtype=bool)
    return labels == labels.dtype.type(key)


# ---- segment statistics, exact -------------------------------------------------------------------------------
def _ints(arrays):
    """Doubles are dyadic rationals: every value of ``arrays`` as a Python int times one common 2**e."""
    flat = [np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
    assert all(np.isfinite(a).all() for a in flat)
    exps = [np.frexp(a)[1][a != 0] for a in flat]
    e = min([int(x.min()) - 53 for x in exps if x.size] or [0])
    out = []
    for a in flat:
        vals = []
        for v in a.tolist():
            m, x = math.frexp(v)
            vals.append(int(m * 2.0 ** 53) << (x - 53 - e) if m else 0)
        out.append(vals)
    return out, e


def _mean_ss(xs, e):
    """(mean, centred sum of squares) of the ints ``xs`` scaled by 2**e, as exact Fractions."""
    n, s, q = len(xs), sum(xs), sum(x * x for x in xs)
    return Fraction(s, n) * Fraction(2) ** e, Fraction(n * q - s * s, n) * Fraction(2) ** (2 * e)


def _pair_slices(ax, lag):
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[ax], hi[ax] = slice(0, -lag), slice(lag, None)
    return tuple(lo), tuple(hi)


def _pairs(mask, raw, ax, lag):
    """(x, y): raw[v] and raw[v + lag along ax] of the pairs with both voxels in the mask."""
    if lag >= mask.shape[ax]:
        return raw[:0, 0, 0], raw[:0, 0, 0]
    lo, hi = _pair_slices(ax, lag)
    sel = mask[lo] & mask[hi]
    return raw[lo][sel], raw[hi][sel]


def segment_stats_exact(labels, key, raw, lag, smooth=None):
    """The 23 columns of exabm4d_segment_stats_dev for the segment ``key`` of one (z, y, x) patch: every sum
    in exact integer / rational arithmetic (sum (x - m)^2 = (n sum x^2 - (sum x)^2) / n holds exactly there),
    each column rounded to float64 once.  Small inputs only."""
    mask = segment_mask(labels, key)
    raw = np.asarray(raw).astype(np.float64)
    row = [0.0] * SEG_STATS_K
    v = raw[mask]
    if v.size:
        if smooth is None:
            (iv,), e = _ints([v])
        else:
            (iv, isv), e = _ints([v, np.asarray(smooth, dtype=np.float64)[mask]])
            mean, ss = _mean_ss([a - b for a, b in zip(iv, isv)], e)
            row[2], row[4] = float(mean), float(ss)
        mean, ss = _mean_ss(iv, e)
        row[0], row[1], row[3] = float(v.size), float(mean), float(ss)
    for ax in range(3):
        x, y = _pairs(mask, raw, ax, lag)
        if not x.size:
            continue
        (ix, iy), e = _ints([x, y])
        n = len(ix)
        mx, sxx = _mean_ss(ix, e)
        my, syy = _mean_ss(iy, e)
        sxy = Fraction(n * sum(a * b for a, b in zip(ix, iy)) - sum(ix) * sum(iy), n) * Fraction(2) ** (2 * e)
        row[5 + 6 * ax:11 + 6 * ax] = [float(n), float(mx), float(my), float(sxx), float(syy), float(sxy)]
    return np.array(row, dtype=np.float64)


# ---- the error a correct fp64 two-pass kernel may make -----------------------------------------------------
# The kernel sums in fp64 in an order of its own (256 strided partial sums, then a tree).  With u = 2^-53,
# ANY summation order of n terms t_i errs by at most (n - 1) u sum |t_i| to first order (Higham, Accuracy and
# Stability of Numerical Algorithms, section 4.2).
#
#   mean.   sum / n: (n - 1) u from the sum and u from the division:  delta = n u mean|r|.
#           The raw - smooth mean sums rounded differences, one more u per term: (n + 1) u mean|h|.
#   Sxx.    The pass centres on a computed mean m' = m + e, |e| <= delta.  Exactly,
#           sum (x - m')^2 = S + n e^2.  A term fl(fl(x - m')^2) carries 3 roundings, the sum n - 1 more:
#           bound = (n + 4) u S + n delta^2   (the 2 spare u cover the second-order terms).
#   Sxy.    Exactly, sum (x - mx')(y - my') = Sxy - ey sum (x - mx) - ex sum (y - my) + n ex ey = Sxy + n ex ey:
#           the first-order cross terms vanish from the VALUE because sum (x - mx) = 0.  They stay in the
#           magnitude the roundings scale with, sum |x - mx'| |y - my'| <= sum |dx dy| + dy_ sum |dx| +
#           dx_ sum |dy| + n dx_ dy_  (dx_, dy_ the two mean bounds):
#           bound = (n + 4) u (sum |dx dy| + dy_ sum |dx| + dx_ sum |dy|) + n dx_ dy_.
#   raw - smooth SS.  Its terms carry a 4th rounding, of h = r - s, which is relative to |h| and not to the
#           centred |h - mh|: the data are perturbed by p_i, |p_i| <= u |h_i|, and the centred sum of squares
#           of perturbed data moves by 2 sum d_i (p_i - pbar) + sum (p_i - pbar)^2
#           <= 2 sqrt(S sum p^2) + sum p^2  (Cauchy-Schwarz).  That is added to the Sxx bound.
# Nothing here comes from what a kernel returned.
def _ss_bound(d, delta):
    n = d.size
    return (n + 4) * U * float(np.sum(d * d)) + n * delta * delta


def segment_stats_bound(labels, key, raw, lag, smooth=None):
    """Per column, the largest |kernel - exact| a correct two-pass fp64 kernel can show (0 for the counts)."""
    mask = segment_mask(labels, key)
    raw = np.asarray(raw).astype(np.float64)
    b = np.zeros(SEG_STATS_K)
    v = raw[mask]
    if v.size:
        n = v.size
        b[1] = n * U * float(np.mean(np.abs(v)))
        b[3] = _ss_bound(v - v.mean(), b[1])
        if smooth is not None:
            h = v - np.asarray(smooth, dtype=np.float64)[mask]
            b[2] = (n + 1) * U * float(np.mean(np.abs(h)))
            sp, s = U * U * float(np.sum(h * h)), float(np.sum((h - h.mean()) ** 2))
            b[4] = _ss_bound(h - h.mean(), b[2]) + 2.0 * math.sqrt(s * sp) + sp
    for ax in range(3):
        x, y = _pairs(mask, raw, ax, lag)
        if not x.size:
            continue
        n = x.size
        ex, ey = n * U * float(np.mean(np.abs(x))), n * U * float(np.mean(np.abs(y)))
        dx, dy = x - x.mean(), y - y.mean()
        cross = float(np.sum(np.abs(dx * dy))) + ey * float(np.sum(np.abs(dx))) + ex * float(np.sum(np.abs(dy)))
        b[5 + 6 * ax:11 + 6 * ax] = [0.0, ex, ey, _ss_bound(dx, ex), _ss_bound(dy, ey),
                                     (n + 4) * U * cross + n * ex * ey]
    return b


COUNT_COLUMNS = (0, 5, 11, 17)


def check_stats(got, want, bound, what=""):
    """Counts equal; every float column within its bound.  Returns the largest error / bound ratio."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(got[list(COUNT_COLUMNS)], want[list(COUNT_COLUMNS)], err_msg=f"{what}: counts")
    err = np.abs(got - want)
    worst = 0.0
    for c in range(SEG_STATS_K):
        if c in COUNT_COLUMNS:
            continue
        assert err[c] <= bound[c], f"{what}: column {c}: got {got[c]!r}, exact {want[c]!r}, " \
                                   f"error {err[c]:.3e} above the bound {bound[c]:.3e}"
        if bound[c] > 0.0:
            worst = max(worst, err[c] / bound[c])
    return worst
