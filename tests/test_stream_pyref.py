"""The numpy restatements of tests/stream_pyref.py against independent formulations (no GPU): exact
rational / decimal arithmetic, fp64 detours that are provably innocuous, np.sort, scipy."""
import struct
from decimal import ROUND_HALF_EVEN, Decimal
from fractions import Fraction

import numpy as np
import pytest

import stream_pyref as P
from oracle import host_oracle as H

F32 = np.float32
EDGES = [-1e30, -3.0, -0.75, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.5, 3.5, 4.5, 1000.5, 1001.5,
         32767.5, 32768.5, 65533.5, 65534.5, 65534.75, 65535.0, 65535.25, 65535.5, 65536.0, 1e30, np.inf,
         -np.inf]
OFFSETS = [0.0, 37.0, -12.5, 36.73, 65536.0]


def nearest_f32(fr):
    """The fp32 nearest (ties to even) to an exact Fraction, by comparing against both neighbours."""
    c = F32(float(fr))         # double rounding cannot move it further than one neighbour
    cands = {float(c), float(np.nextafter(c, F32(-np.inf))), float(np.nextafter(c, F32(np.inf)))}
    best = min(cands, key=lambda v: (abs(Fraction(v) - fr), int(F32(v).view(np.uint32)) & 1))
    return F32(best)


def test_counts_from_u16_is_one_correctly_rounded_subtraction():
    v = np.arange(65536, dtype=np.uint16)
    for off in OFFSETS + [0.1, 1e-3, 12345.678]:
        got = P.counts_from_u16(v, off)
        assert got.dtype == F32
        # both operands have <= 24 significant bits within 2^-150 .. 2^17: their fp64 difference is exact
        want = (v.astype(np.float64) - np.float64(F32(off))).astype(F32)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    rng = np.random.default_rng(0)
    for x, off in zip(rng.integers(0, 65536, 40), rng.uniform(-100, 100, 40)):
        fr = Fraction(int(x)) - Fraction(float(F32(off)))
        assert P.counts_from_u16(np.array([x], np.uint16), off)[0] == nearest_f32(fr)


def decimal_quantise(x):
    d = min(max(Decimal(float(x)), Decimal(0)), Decimal(65535))
    return int(d.quantize(Decimal(1), rounding=ROUND_HALF_EVEN))


def test_quantise_rounds_half_to_even_and_clamps():
    finite = [e for e in EDGES if np.isfinite(e)]
    ties = [k + 0.5 for k in range(0, 70)] + [k + 0.5 for k in range(65500, 65536)]
    x = np.array(finite + ties, dtype=F32)
    got = P.quantise_u16(x)
    assert got.dtype == np.uint16
    assert got.tolist() == [decimal_quantise(v) for v in x]
    assert P.quantise_u16(np.array([np.inf, -np.inf], F32)).tolist() == [65535, 0]
    assert P.quantise_u16(np.array([0.5, 1.5, 2.5, 65534.5], F32)).tolist() == [0, 2, 2, 65534]
    assert P.quantise_u16(np.array([300.5, 301.5], F32), max_count=301.0).tolist() == [300, 301]


def test_round_counts_and_normalize_u16_against_exact_arithmetic():
    rng = np.random.default_rng(1)
    num = np.concatenate([rng.normal(300, 500, 300), np.arange(1, 200, 2.0), [1e30, -1e30, 0.0]]).astype(F32)
    den = np.concatenate([rng.uniform(0.3, 9, 300), np.full(100, 2.0), [1e-30, 1e-30, 5.0]]).astype(F32)
    for off in OFFSETS:
        o32 = F32(off)
        got = P.normalize_u16(num, den, off)
        rc = P.round_counts(num, off)
        for i in range(num.size):
            q = Fraction(float(num[i])) / Fraction(float(den[i]))
            if abs(q) > Fraction(2) ** 127:       # the quotient overflows to +-inf
                want = 65535 if q > 0 else 0
            else:
                s = nearest_f32(Fraction(float(nearest_f32(q))) + Fraction(float(o32)))
                want = decimal_quantise(s)
            assert int(got[i]) == want, (i, off)
            s = nearest_f32(Fraction(float(num[i])) + Fraction(float(o32)))
            want_rc = nearest_f32(Fraction(decimal_quantise(s)) - Fraction(float(o32)))
            assert rc[i] == want_rc, (i, off)
    assert rc.dtype == F32 and got.dtype == np.uint16


def test_normalize_is_the_fp32_quotient_with_np_clip():
    rng = np.random.default_rng(2)
    num, den = rng.normal(0, 100, 500).astype(F32), rng.uniform(-3, 3, 500).astype(F32)
    # fp64 holds more than 2 * 24 + 2 bits: rounding the fp64 quotient to fp32 is the fp32 quotient
    want = (num.astype(np.float64) / den.astype(np.float64)).astype(F32)
    np.testing.assert_array_equal(P.normalize(num, den), want)
    np.testing.assert_array_equal(P.normalize(num, den, (-7.5, 20.0)), np.minimum(np.maximum(want, F32(-7.5)), F32(20)))
    assert P.normalize(np.array([1.0], F32), np.array([0.0], F32))[0] == np.inf


def test_tile_finalize_linear_by_hand():
    cfg = {"kind": "linear", "params": {"mn": 35.0, "mx": 1000.0, "clip": 8.0}}
    acc = np.array([0.0, 0.5, 1.0, 3.0, 2.0, 1e30, -4.0], F32)
    wgt = np.array([0.0, 1.0, 1.0, 3.0, 4.0, 1.0, 2.0], F32)
    y = acc / (wgt + F32(1e-8))
    c = y * F32(965.0) + F32(35.0)
    want = np.rint(np.minimum(np.maximum(c, F32(0)), F32(65535))).astype(np.uint16)
    np.testing.assert_array_equal(P.tile_finalize(cfg, acc, wgt), want)
    assert want.tolist()[:3] == [35, 518, 1000] and want[5] == 65535 and want[6] == 0


def python_key(v):
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~bits) & 0xFFFFFFFFFFFFFFFF if bits >> 63 else bits | (1 << 63)


SPECIAL = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, np.finfo(np.float64).max,
           -np.finfo(np.float64).max, 1.0, -1.0, 1.0000000000000002, 65535.0, 1e-40, -1e-40]


def test_keys_order_like_the_values():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(0, 1e3, 3000), rng.normal(0, 1e-300, 100), SPECIAL])
    keys = P.f64_keys(x)
    assert [int(k) for k in keys[-len(SPECIAL):]] == [python_key(float(v)) for v in SPECIAL]
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(x[order], np.sort(x))            # ascending keys <=> ascending values
    assert keys[x.size - len(SPECIAL) + 1] < keys[x.size - len(SPECIAL)]       # -0.0 sorts before +0.0
    for k, v in zip(keys, x):
        back = P.key_to_f64(k)
        assert back == v and np.signbit(back) == np.signbit(v)
    for dt in (np.uint16, np.float32):
        y = rng.integers(0, 65536, 500).astype(dt)
        np.testing.assert_array_equal(P.f64_keys(y), P.f64_keys(y.astype(np.float64)))
    c = float(x[17])
    np.testing.assert_array_equal(P.f64_keys(x, center=c), P.f64_keys(np.abs(x - c)))
    assert int(P.f64_keys(x, center=c)[17]) == 1 << 63             # |v - v| = +0


def test_digit_histograms_recombine_into_a_radix_selection():
    rng = np.random.default_rng(4)
    with np.errstate(over="ignore"):          # +-max double become +-inf as float32
        x = np.concatenate([rng.normal(100, 400, 4000), SPECIAL, np.full(9, 7.25)]).astype(np.float32)
    keys = P.f64_keys(x)
    srt = np.sort(x.astype(np.float64))
    for k in (0, 1, 17, x.size // 2, x.size - 2, x.size - 1):
        kk, prefix = k, 0
        for digit in range(4):
            hist = P.key_digit_histogram(keys, digit, prefix)
            if digit:      # the digit histogram under a prefix sums to that prefix's bin one digit up
                assert int(hist.sum()) == int(P.key_digit_histogram(keys, digit - 1, prefix >> 16)[prefix & 0xFFFF])
            cum = np.cumsum(hist.astype(np.int64))
            d = int(np.searchsorted(cum, kk, side="right"))
            kk -= int(cum[d - 1]) if d else 0
            prefix = (prefix << 16) | d
        got = P.key_to_f64(prefix)
        assert got == srt[k] and np.signbit(got) == np.signbit(srt[k])
    assert int(P.key_digit_histogram(keys, 0).sum()) == x.size


def test_i32_symbols():
    v = np.array([0, 1, -1, 32766, 32767, 32768, 32769, -32766, -32767, -32768, -32769, 2 ** 31 - 1, -2 ** 31],
                 dtype=np.int32)
    want = [32768, 32769, 32767, 65534, 65535, 0, 0, 2, 1, 0, 0, 0, 0]
    assert P.i32_symbols(v).tolist() == want
    assert [0 if abs(int(a)) > 32767 else int(a) + 32768 for a in v] == want
    hist = P.i32_symbol_histogram(v)
    assert hist.dtype == np.uint64 and hist.size == 65536 and int(hist[0]) == 6 and int(hist.sum()) == v.size


def test_masked_error_stats_columns():
    p = np.array([1.0, 5.0, 2.0, 9.0, 4.0], np.float32)
    r = np.array([0, 7, 2, 1, 10], np.uint16)
    m = np.array([1, 0, 0, 2, 0], np.uint8)
    np.testing.assert_array_equal(P.masked_error_stats(p, r, m, 4.0), [9.0, 8.0, 2.0, 1.0, 9.0, 10.0, 8.0])
    np.testing.assert_array_equal(P.masked_error_stats(p, r, None, 4.0), [0.0, 17.0, 0.0, 2.0, 9.0, 10.0, 8.0])
    np.testing.assert_array_equal(P.masked_error_stats(p, r, None, np.inf)[3], 0.0)


@pytest.mark.parametrize("shape,window", [((6, 5, 7), 3), ((5, 3, 2), 4), ((9, 8, 10), 16), ((4, 4, 4), 1)])
def test_direct_ssim_agrees_with_scipy_on_benign_data(shape, window):
    """Benign data (mean 300, sd 60): nothing cancels, so scipy's running sums and the direct window sums
    agree to a few fp64 roundings -- this pins the window placement and the boundary rule."""
    rng = np.random.default_rng(sum(shape) + window)
    a = rng.normal(300, 60, shape)
    b = a + rng.normal(0, 25, shape)
    rangev = max(a.max() - a.min(), b.max() - b.min())
    c1, c2 = (0.01 * rangev) ** 2, (0.03 * rangev) ** 2
    assert P.ssim3d_direct(a, b, window, c1, c2) == pytest.approx(H.ssim3d(a, b, window_size=window), rel=1e-11)
    assert P.ssim3d_direct(a, a, window, c1, c2) == pytest.approx(1.0, abs=1e-6)
