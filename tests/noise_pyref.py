"""Plain numpy restatement of the noise table and of the estimators on it: int64 arithmetic and
np.add.at for uint16 input, float32 with the specification's association for float32 input."""
import math

import numpy as np

LEVELS = 49
BINS = 4096
S_MAX = 8 * 65535
MAD_TO_SIGMA = 0.674489750196082 * math.sqrt(8.0)


def level_of(s):
    """Quarter-octave level of the cell sums ``s`` (int64 array)."""
    t = (np.asarray(s, dtype=np.int64) >> 3) + 16
    e = np.floor(np.log2(t.astype(np.float64))).astype(np.int64)      # t < 2^17: exact
    q = (t >> (e - 2)) & 3
    return 4 * (e - 4) + q


def _cells(vol):
    """The eight corner arrays v[dz][dy][dx] of the 2x2x2 cells at even coordinates, trailing odd slices ignored."""
    nz, ny, nx = (n // 2 * 2 for n in vol.shape)
    v = vol[:nz, :ny, :nx]
    return [[[v[dz::2, dy::2, dx::2] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]


def cell_values(vol):
    """(s, m, valid) per cell as flat int64 / int64 / bool arrays; m = -1 marks |d| >= 2^24 (last bin)."""
    vol = np.asarray(vol)
    assert vol.ndim == 3 and min(vol.shape) >= 2
    c = _cells(vol)
    if vol.dtype == np.uint16:
        s = np.zeros(c[0][0][0].shape, dtype=np.int64)
        d = np.zeros(c[0][0][0].shape, dtype=np.int64)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    s += c[dz][dy][dx].astype(np.int64)
                    d += (-1) ** (dz + dy + dx) * c[dz][dy][dx].astype(np.int64)
        return s.reshape(-1), np.abs(d).reshape(-1), np.ones(s.size, dtype=bool)
    assert vol.dtype == np.float32
    v = [[[np.ascontiguousarray(c[dz][dy][dx]) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((v[0][0][0] + v[0][0][1]) + (v[0][1][0] + v[0][1][1])) + ((v[1][0][0] + v[1][0][1]) + (v[1][1][0] + v[1][1][1]))
        d = ((v[0][0][0] - v[0][0][1]) - (v[0][1][0] - v[0][1][1])) - ((v[1][0][0] - v[1][0][1]) - (v[1][1][0] - v[1][1][1]))
    assert s.dtype == np.float32 and d.dtype == np.float32
    s, d = s.reshape(-1), d.reshape(-1)
    valid = np.isfinite(s) & np.isfinite(d)
    s = np.where(valid, s, np.float32(0))
    d = np.where(valid, d, np.float32(0))
    si = np.clip(np.floor(s), 0, S_MAX).astype(np.int64)
    ad = np.abs(d)
    big = ad >= np.float32(2.0 ** 24)
    m = np.where(big, -1, np.rint(np.where(big, np.float32(0), ad)).astype(np.int64))     # np.rint: half to even
    return si, m, valid


def table(vol, shift=0):
    """(hist[LEVELS, BINS] uint64, sum_s[LEVELS] uint64, skipped) of a 3-D volume, or of a 4-D batch of patches
    as one population."""
    vol = np.asarray(vol)
    assert 0 <= shift <= 6
    hist = np.zeros((LEVELS, BINS), dtype=np.int64)
    sum_s = np.zeros(LEVELS, dtype=np.int64)
    skipped = 0
    for patch in (vol if vol.ndim == 4 else [vol]):
        s, m, valid = cell_values(patch)
        skipped += int(np.count_nonzero(~valid))
        s, m = s[valid], m[valid]
        lv = level_of(s)
        b = np.where(m < 0, BINS - 1, np.minimum(m >> shift, BINS - 1))
        np.add.at(hist, (lv, b), 1)
        np.add.at(sum_s, lv, s)
    return hist.astype(np.uint64), sum_s.astype(np.uint64), skipped


def sigma_of(row, shift):
    """Interpolated median of |d| over a row of the table, over 0.6745 sqrt(8); NaN when the row is empty or the
    median lies in the last bin."""
    row = [int(x) for x in row]
    n = sum(row)
    if n == 0:
        return float("nan")
    half = n / 2.0
    below = 0
    for b, cnt in enumerate(row):
        if below + cnt >= half:
            break
        below += cnt
    if b == BINS - 1:
        return float("nan")
    w = float(1 << shift)
    lower = b * w - 0.5 if b else 0.0
    upper = (b + 1) * w - 0.5
    median = lower + (half - float(below)) / float(row[b]) * (upper - lower)
    return median / MAD_TO_SIGMA


def auto_table(vol, min_cells=512):
    """The table at the smallest shift at which neither the pooled row nor a level with >= min_cells cells has its
    median in the last bin; (hist, sum_s, skipped, shift)."""
    for shift in range(7):
        hist, sum_s, skipped = table(vol, shift)
        rows = [hist.sum(axis=0)] + [hist[lv] for lv in range(LEVELS) if int(hist[lv].sum()) >= min_cells]
        if not any(int(r.sum()) > 0 and math.isnan(sigma_of(r, shift)) for r in rows):
            break
    return hist, sum_s, skipped, shift


def estimate_sigma(vol):
    hist, _, _, shift = auto_table(vol)
    return sigma_of(hist.sum(axis=0), shift)


def noise_curve(vol, min_cells=512):
    hist, sum_s, _, shift = auto_table(vol, min_cells)
    mean, sig, cells = [], [], []
    for lv in range(LEVELS):
        n = int(hist[lv].sum())
        if n >= max(1, min_cells):
            s = sigma_of(hist[lv], shift)
            if not math.isnan(s):
                mean.append(float(sum_s[lv]) / (8.0 * float(n)))
                sig.append(s)
                cells.append(n)
    return np.array(mean, dtype=np.float64), np.array(sig, dtype=np.float64), np.array(cells, dtype=np.int64)


def fit_poisson_gaussian(mean, sigma, cells, offset):
    """Weighted least squares sigma^2 = a mean + c with weights cells / sigma^4."""
    mean, sigma, cells = (np.asarray(v, dtype=np.float64) for v in (mean, sigma, cells))
    ok = sigma > 0.0
    mean, sigma, cells = mean[ok], sigma[ok], cells[ok]
    if mean.size < 3:
        raise ValueError("fewer than three usable intensity levels")
    y = sigma * sigma
    w = cells / (y * y)
    wsum = np.sum(w)
    xm = np.sum(w * mean) / wsum
    ym = np.sum(w * y) / wsum
    a = np.sum(w * (mean - xm) * (y - ym)) / np.sum(w * (mean - xm) * (mean - xm))
    c = ym - a * xm
    if not a > 0.0:
        raise ValueError("the fitted slope is not positive")
    return {"gain": float(a), "read_noise": float(math.sqrt(max(c + a * float(offset), 0.0))),
            "offset": float(offset)}


def estimate_poisson_gaussian(vol, offset, min_cells=512):
    return fit_poisson_gaussian(*noise_curve(vol, min_cells), offset)
