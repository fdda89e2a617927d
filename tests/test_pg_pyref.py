"""tests/pg_pyref.py -- the specification of the Poisson-Gaussian stabilisation -- checked on the
CPU: against this repo's restatement of the reference's AnscombeTransform, against the closed form in float64,
for monotonicity, and, composed with the oracle's fp32 BM4D, for what the feature is for: PSNR against the
scalar-sigma pipeline, background bias of the inverses, and noise of unit sigma after the forward."""
import math

import numpy as np
import pytest

import noise_pyref
import pg_pyref as P
from oracle import host_oracle as H
from util import psnr, synth_volume

F32 = np.float32
PARAMS = [(4.0, 6.0, 37.0), (20.0, 3.0, 37.0), (1.5, 8.0, 100.0), (1.0, 0.0, 0.0)]
KINDS = ["closed_form", "asymptotic", "algebraic"]


def top_of(c):
    return float(P.forward(np.array([65535], np.uint16), c)[0])


@pytest.mark.parametrize("params", PARAMS)
def test_agrees_with_the_anscombe_transform(params):
    """forward * (1 / norm) is AnscombeTransform.forward, and the two closed inverses are its inverse_float (1/8
    with unbiased_inverse, 3/8 without) on d = y * norm -- the one operation the transform has and the
    un-normalised form does not -- bit for bit."""
    gain, rn, off = params
    x = np.arange(65536, dtype=np.uint16)
    D = P.forward(x, params)
    for unbiased, kind in ((True, "asymptotic"), (False, "algebraic")):
        tf = H.TransformOracle({"kind": "anscombe", "params": {"gain": gain, "read_noise": rn, "offset": off,
                                                                "unbiased_inverse": unbiased}})
        y = tf.forward(x)
        np.testing.assert_array_equal(D / F32(tf.norm), y)
        d = np.maximum(y, F32(0.0)) * F32(tf.norm)
        np.testing.assert_array_equal(P.inverse_float(d, params, kind), tf.inverse_float(y))
        np.testing.assert_array_equal(P.inverse(d, params, kind), tf.inverse(y))


def test_forward_is_the_anscombe_transform_at_unit_gain():
    x = np.arange(65536, dtype=np.uint16)
    np.testing.assert_array_equal(P.forward(x, (1.0, 0.0, 0.0)), F32(2.0) * np.sqrt(x.astype(F32) + F32(3.0 / 8.0)))
    c = P.Consts(1.0, 0.0, 0.0)
    assert c.d0 == F32(2.0) * np.sqrt(F32(3.0 / 8.0)) and c.s2 == 0.0


def test_closed_form_float64_and_float32():
    """In float64 at s2 = 0 the closed form vanishes at d0 = 2 sqrt(3/8): 3/8 + 1/4 - 11/12 + 5/12 - 1/8 = 0.

    float32 against float64 (exact constants) on 200 001 values of D from 0 to the stabilised 65535.  The float32
    chain has about twenty rounded steps (d^2, d^3, three quotients, five sums, the product with the gain, the
    offset, the constants k1, k3, s2 and d0), each at most 2^-24 of a term that is itself at most
    scale = gain (d^2/4 + (11/8)/d^2 + s2) + |offset|; so |est32 - est64| <= 24 * 2^-24 * scale.  Measured: at
    most 4.3 * 2^-24 * scale over the four parameter sets (0.0099 counts at gain 20)."""
    y0 = float(P.closed_form_f64(2.0 * math.sqrt(3.0 / 8.0), 1.0, 0.0, clamp=False))
    assert abs(y0) <= 8 * 2.0 ** -53
    for params in PARAMS:
        c = P.Consts(*params)
        D = np.linspace(0.0, top_of(c), 200001).astype(F32)
        e32 = P.inverse_float(D, c, "closed_form").astype(np.float64)
        e64 = P.closed_form_f64(D.astype(np.float64), *params)
        d = np.maximum(D.astype(np.float64), float(c.d0))
        scale = params[0] * (d * d / 4.0 + (11.0 / 8.0) / (d * d) + float(c.s2)) + abs(params[2])
        units = np.abs(e32 - e64) / (scale * 2.0 ** -24)
        print(f"{params}: max |est32 - est64| = {np.abs(e32 - e64).max():.5f} counts, {units.max():.2f} units")
        assert units.max() <= 24.0
        assert np.all(e64 >= params[2])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params", PARAMS)
def test_inverse_is_monotone(params, kind):
    """Non-decreasing in D, as floats and as counts: below d0 = 2 sqrt(3/8) the closed form's 1/d^3 term would
    turn it round, hence the clamp."""
    c = P.Consts(*params)
    D = np.concatenate([np.linspace(-1.0, top_of(c) + 1.0, 100001).astype(F32),
                        [F32(0.0), c.d0, np.nextafter(c.d0, F32(np.inf)), np.nextafter(c.d0, F32(-np.inf))]])
    D = np.sort(D.astype(F32))
    est = P.inverse_float(D, c, kind)
    assert np.all(np.diff(est) >= 0.0)
    assert np.all(np.diff(P.quantise(est).astype(np.int64)) >= 0)
    if kind == "closed_form":
        assert np.all(est[D <= c.d0] == est[D == c.d0][0])
        # without the clamp it does turn round: the float64 form rises again towards D = 0
        assert P.closed_form_f64(0.05, params[0], params[1], clamp=False) > \
            P.closed_form_f64(float(c.d0), params[0], params[1], clamp=False)


def pg_case(gain, rn, off, shape):
    _, clean = synth_volume(shape, seed=3, pedestal=off)
    return clean, P.pg_volume(clean, gain, rn, off, np.random.default_rng(7))


def test_quality_against_the_pooled_sigma(oracle):
    """Gain 4, read noise 6, offset 37 on synth_volume((40, 40, 40), seed=3): the stabilised composition against
    the scalar-sigma pipeline at the pooled estimate -- what sigma="auto" gives.  Measured with the oracle:
    52.15 dB against 43.33 dB (pooled sigma 6.19), a gap of 8.82 dB; at least half of it is asserted."""
    gain, rn, off = PARAMS[0]
    clean, v = pg_case(gain, rn, off, (40, 40, 40))
    peak = clean.max() - off
    pooled = noise_pyref.estimate_sigma(v)
    p_scalar = psnr(oracle.bm4d_u16(v, pooled, off), clean, peak)
    p_stab = psnr(P.denoise(oracle, v, PARAMS[0]), clean, peak)
    print(f"stabilised {p_stab:.2f} dB, scalar sigma {pooled:.2f}: {p_scalar:.2f} dB, gap {p_stab - p_scalar:.2f} dB")
    assert p_stab - p_scalar >= 0.5 * 8.82


def test_background_bias_of_the_inverses(oracle):
    """Gain 20, read noise 3, offset 37 (few photons): mean error over the voxels with clean < offset + 1.
    Measured with the oracle: closed form -0.002 counts, asymptotic +4.91 counts."""
    gain, rn, off = PARAMS[1]
    clean, v = pg_case(gain, rn, off, (40, 36, 44))
    est = oracle.bm4d(P.forward(v, PARAMS[1]), 1.0, stages=2)
    bg = clean < off + 1.0
    bias = {k: float(np.mean(P.inverse(est, PARAMS[1], k)[bg].astype(np.float64) - clean[bg])) for k in KINDS}
    print("background bias, counts:", bias, "over", int(bg.sum()), "voxels")
    assert abs(bias["closed_form"]) < 0.5
    assert bias["asymptotic"] > 2.0


def test_forward_stabilises_the_noise():
    """Seven slabs of constant clean signal (offset + 0 ... 40000 counts) under gain 4, read noise 6: the noise
    curve of noise_pyref on D -- on 64 D, an exact scaling that keeps the table's integer bins fine -- for the
    levels with at least 512 cells (six: the zero-photon slab straddles two levels).  Measured on this input: sigma
    between 0.950 and 1.007; asserted with a margin of 0.03 on either side."""
    gain, rn, off = PARAMS[0]
    levels = off + np.array([0.0, 40.0, 160.0, 640.0, 2560.0, 10240.0, 40000.0])
    clean = np.repeat(levels, 8)[:, None, None] * np.ones((1, 32, 32))
    v = P.pg_volume(clean, gain, rn, off, np.random.default_rng(11))
    D = P.forward(v, PARAMS[0])
    mean, sigma, cells = noise_pyref.noise_curve(D * F32(64.0), min_cells=512)
    sigma = sigma / 64.0
    print("levels (D):", np.round(mean / 64.0, 2), "sigma:", np.round(sigma, 4), "cells:", cells)
    assert sigma.size >= 5
    assert 0.950 - 0.03 <= sigma.min() and sigma.max() <= 1.007 + 0.03
    # the counts themselves are nowhere near one sigma: 6 at the pedestal, 400 at the top
    _, raw_sigma, _ = noise_pyref.noise_curve(v, min_cells=512)
    assert raw_sigma.max() / raw_sigma.min() > 20.0
