"""Plain numpy restatements of the small streaming and statistics operations of include/exabm4d.h,
one function per operation, written from the header's comments.

TEST INFRASTRUCTURE ONLY.  Every step is one explicit ``np.float32`` / ``np.float64`` / integer
operation, so each result is *the* value of the operation (a correctly rounded IEEE step), not an
approximation of it: the GPU tests compare with ``assert_array_equal``.  NaN inputs are outside these
functions' domain (a C cast of NaN to an integer has no numpy counterpart).

tests/test_stream_pyref.py checks every function here against an independent formulation without a GPU.
"""
import numpy as np

from oracle.host_oracle import TransformOracle

F32 = np.float32
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore")


def _f32a(x):
    return np.ascontiguousarray(x, dtype=F32)


# ---- exabm4d_counts_from_u16_dev ----------------------------------------------------------------------
def counts_from_u16(v, offset):
    """out = (float)in - offset: the uint16 count widened exactly, one fp32 subtraction."""
    v = np.asarray(v)
    assert v.dtype == np.uint16
    return v.astype(F32) - F32(offset)


# ---- the quantiser shared by normalize_u16 / round_counts / the inverse transforms ----------------------
def quantise_u16(c, max_count=65535.0):
    """uint16(rint(clamp(c, 0, max_count))), rint rounding half to even (np.clip then np.rint)."""
    c = np.clip(_f32a(c), F32(0.0), F32(max_count))
    return np.rint(c).astype(np.uint16)


# ---- exabm4d_round_counts_f32_dev ----------------------------------------------------------------------
def round_counts(x, offset):
    """out = (float)rint(clamp(in + offset, 0, 65535)) - offset."""
    off = F32(offset)
    with np.errstate(**_QUIET):
        q = quantise_u16(_f32a(x) + off)
    return q.astype(F32) - off


# ---- exabm4d_normalize_u16_dev -------------------------------------------------------------------------
def normalize_u16(num, den, offset):
    """out = uint16(rint(clamp(num / den + offset, 0, 65535))): fp32 quotient, fp32 sum."""
    with np.errstate(**_QUIET):
        return quantise_u16(_f32a(num) / _f32a(den) + F32(offset))


# ---- exabm4d_normalize_dev -----------------------------------------------------------------------------
def normalize(num, den, clip=None):
    """out = num / den in fp32, then np.clip to [lo, hi] when a clip range is given."""
    with np.errstate(**_QUIET):
        out = _f32a(num) / _f32a(den)
    if clip is not None:
        out = np.clip(out, F32(clip[0]), F32(clip[1]))
    return out


# ---- exabm4d_tile_finalize_u16_dev ---------------------------------------------------------------------
def tile_finalize(cfg, acc, wgt):
    """out = transform.inverse(accum_pred / (accum_wgt + 1e-8f)); the inverse is the transforms' bit-exact
    oracle."""
    with np.errstate(**_QUIET):
        y = _f32a(acc) / (_f32a(wgt) + F32(1e-8))
        return TransformOracle(cfg).inverse(y)


# ---- exabm4d_key_histogram_dev -------------------------------------------------------------------------
def f64_keys(x, center=None):
    """Order-preserving 64-bit keys of the values widened to fp64 (of |v - center| when a centre is given):
    key = bits | 2^63 for values without the sign bit, ~bits for those with it."""
    v = np.asarray(x).astype(np.float64).reshape(-1)
    if center is not None:
        with np.errstate(**_QUIET):
            v = np.abs(v - np.float64(center))
    bits = np.ascontiguousarray(v).view(np.uint64)
    neg = (bits >> np.uint64(63)) != 0
    return np.where(neg, ~bits, bits | np.uint64(1 << 63))


def key_digit_histogram(keys, digit, prefix=0):
    """hist[65536] of digit `digit` (0 = most significant 16 bits .. 3) of the keys whose higher digits
    equal `prefix`."""
    keys = np.asarray(keys, dtype=np.uint64)
    shift = 48 - 16 * digit
    if digit > 0:
        keys = keys[(keys >> np.uint64(shift + 16)) == np.uint64(prefix)]
    d = (keys >> np.uint64(shift)) & np.uint64(0xFFFF)
    return np.bincount(d.astype(np.int64), minlength=65536).astype(np.uint64)


def key_to_f64(key):
    """The fp64 value a key stands for."""
    key = int(key)
    bits = key ^ (1 << 63) if key >> 63 else ~key & 0xFFFFFFFFFFFFFFFF
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


# ---- exabm4d_i32_symbol_histogram_dev ------------------------------------------------------------------
def i32_symbols(idx):
    """bin v + 32768 for -32767 <= v <= 32767, bin 0 (the escape symbol) for everything else."""
    v = np.asarray(idx)
    assert v.dtype == np.int32
    v = v.astype(np.int64)
    return np.where((v >= -32767) & (v <= 32767), v + 32768, 0)


def i32_symbol_histogram(idx):
    return np.bincount(i32_symbols(idx).reshape(-1), minlength=65536).astype(np.uint64)


# ---- exabm4d_masked_error_stats_dev --------------------------------------------------------------------
def masked_error_stats(pred, ref, mask, thr):
    """The seven columns with the two sums as EXACT fractions' nearest doubles (math.fsum): { sum |p - r|
    over foreground, the same over background, foreground voxels, background voxels with p > thr, max p,
    max r, max |p - r| }; mask None = all background."""
    import math
    p = np.asarray(pred).astype(np.float64).reshape(-1)
    r = np.asarray(ref).astype(np.float64).reshape(-1)
    fg = np.zeros(p.size, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    with np.errstate(**_QUIET):
        e = np.abs(p - r)
    return np.array([math.fsum(e[fg]), math.fsum(e[~fg]), float(np.count_nonzero(fg)),
                     float(np.count_nonzero(p[~fg] > thr)), p.max(), r.max(), e.max()])


# ---- exabm4d_ssim3d_dev --------------------------------------------------------------------------------
def ssim3d_direct(a, b, window, c1, c2):
    """Mean SSIM with every window sum taken directly from the reflect-padded volume (no running sums), in
    np.longdouble: window i - w/2 .. i + w - w/2 - 1 per axis, scipy's "reflect" boundary (the edge voxel is
    repeated: np.pad's "symmetric")."""
    L = np.longdouble
    a, b = np.asarray(a).astype(L), np.asarray(b).astype(L)
    w = int(window)
    left = w // 2
    right = w - 1 - left

    def pad(v):      # windows wider than an axis reflect repeatedly, in np.pad as in scipy
        return np.pad(v, [(left, right)] * 3, mode="symmetric")

    def box(v):
        p = pad(v)
        out = np.zeros(v.shape, dtype=L)
        nz, ny, nx = v.shape
        for dz in range(w):
            for dy in range(w):
                for dx in range(w):
                    out += p[dz:dz + nz, dy:dy + ny, dx:dx + nx]
        return out / L(w) ** 3

    m1, m2 = box(a), box(b)
    v1, v2, v12 = box(a * a) - m1 * m1, box(b * b) - m2 * m2, box(a * b) - m1 * m2
    num = (2 * m1 * m2 + L(c1)) * (2 * v12 + L(c2))
    den = (m1 * m1 + m2 * m2 + L(c1)) * (v1 + v2 + L(c2))
    return float(np.mean(num / (np.maximum(den, L(1e-8)) + L(1e-6))))
