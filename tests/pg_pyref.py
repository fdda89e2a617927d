"""Plain numpy restatement of the Poisson-Gaussian stabilisation: the un-normalised generalised
Anscombe transform of uint16 counts, its three inverses and the quantiser.  The order of the operations written here
IS the specification; the kernels mirror it (csrc/elementwise_kernels.hip: pg_forward, pg_inverse).

Every array operation is one float32 operation.  Every constant is formed in float64 from the float32 values of
gain, read noise and offset (the C struct carries floats) and rounded once.  Composed with the oracle's fp32
pipeline, ``quantise(inverse(oracle.bm4d(forward(v), 1.0, stages)))`` is what ``exabm4d_denoise_pg_u16_dev``
returns, bit for bit.

The closed form is Makitalo & Foi's: the approximation I0 of the exact unbiased inverse of the Anscombe transform
of Poisson data, minus (read_noise / gain)^2, floored at 0.  I0 is defined from d0 = 2 sqrt(3/8) upwards -- the
transform of zero photons -- and d is clamped there.  (d0 is NOT the transform of the pedestal 2 sqrt(3/8 + s2):
the two agree at read noise 0 only, and a denoised background lies BELOW the transformed pedestal, by Jensen's
inequality, so a clamp there floors every background voxel at offset + gain / 4; DESIGN.md 5.10 has the figures.)"""
import math

import numpy as np

F32 = np.float32
INVERSES = {"algebraic": 0, "asymptotic": 1, "closed_form": 2}


class Consts:
    """The float32 constants of one (gain, read_noise, offset)."""

    def __init__(self, gain, read_noise, offset):
        self.gain, self.read_noise, self.off = F32(gain), F32(read_noise), F32(offset)
        g, r = float(self.gain), float(self.read_noise)
        assert g > 0.0 and r >= 0.0
        self.c38g2 = F32((3.0 / 8.0) * g * g)
        self.rn2 = F32(r * r)
        self.two_over_gain = F32(2.0 / g)
        self.cg2 = {0: F32((3.0 / 8.0) * g * g), 1: F32((1.0 / 8.0) * g * g)}
        self.s2 = F32((r / g) * (r / g))
        self.k1 = F32(math.sqrt(1.5) / 4.0)
        self.k2 = F32(11.0 / 8.0)
        self.k3 = F32(5.0 * math.sqrt(1.5) / 8.0)
        # where the Poisson inverse starts: the transform of zero photons at unit gain without read noise
        self.d0 = F32(2.0 * math.sqrt(3.0 / 8.0))


def _consts(params):
    if isinstance(params, Consts):
        return params
    if isinstance(params, dict):
        return Consts(params["gain"], params["read_noise"], params["offset"])
    return Consts(*params)


def forward(x, params):
    """D, noise of unit sigma: a = g (x - o); a = a + 3 g^2 / 8; a = a + r^2; D = (2 / g) sqrt(max(a, 0))."""
    c = _consts(params)
    x = np.asarray(x).astype(F32)
    a = c.gain * (x - c.off)
    a = a + c.c38g2
    a = a + c.rn2
    out = c.two_over_gain * np.sqrt(np.maximum(a, F32(0.0)))
    assert out.dtype == F32
    return out


def inverse_float(D, params, inverse="closed_form"):
    """The estimate in counts, float32, before the quantiser."""
    c = _consts(params)
    kind = INVERSES[inverse] if isinstance(inverse, str) else int(inverse)
    D = np.asarray(D, dtype=F32)
    if kind in (0, 1):
        h = np.maximum(D, F32(0.0)) * c.gain / F32(2.0)
        u = (h * h - c.cg2[kind]) - c.rn2
        out = c.off + u / c.gain
    elif kind == 2:
        d = np.maximum(D, c.d0)
        d2 = d * d
        d3 = d2 * d
        y = d2 * F32(0.25)
        y = y + c.k1 / d
        y = y - c.k2 / d2
        y = y + c.k3 / d3
        y = y - F32(0.125)
        y = y - c.s2
        out = c.off + c.gain * np.maximum(y, F32(0.0))
    else:
        raise ValueError("inverse must be 0, 1 or 2")
    assert out.dtype == F32
    return out


def quantise(c):
    """clip to [0, 65535], round half to even, uint16"""
    return np.rint(np.clip(np.asarray(c, dtype=F32), F32(0.0), F32(65535.0))).astype(np.uint16)


def inverse(D, params, inverse="closed_form"):
    return quantise(inverse_float(D, params, inverse))


def closed_form_f64(D, gain, read_noise, offset=0.0, clamp=True):
    """The closed form in float64 from the exact constants (not the float32 ones): what the float32 chain
    approximates.  ``clamp=False`` leaves out max(D, d0) and max(y, 0) and returns y itself."""
    g, r = float(gain), float(read_noise)
    s2 = (r / g) ** 2
    d = np.asarray(D, dtype=np.float64)
    if clamp:
        d = np.maximum(d, 2.0 * math.sqrt(3.0 / 8.0))
    y = d * d / 4.0 + (math.sqrt(1.5) / 4.0) / d - (11.0 / 8.0) / (d * d) + (5.0 * math.sqrt(1.5) / 8.0) / (d * d * d) \
        - 1.0 / 8.0 - s2
    return float(offset) + g * np.maximum(y, 0.0) if clamp else y


def pg_volume(clean, gain, read_noise, offset, rng):
    """uint16 counts = gain Poisson((clean - offset) / gain) + N(offset, read_noise), rounded and clipped."""
    lam = np.maximum(np.asarray(clean, dtype=np.float64) - offset, 0.0) / gain
    v = gain * rng.poisson(lam) + rng.normal(offset, read_noise, lam.shape)
    return np.rint(np.clip(v, 0, 65535)).astype(np.uint16)


def denoise(oracle, vol_u16, params, inverse_kind="closed_form", stages=2):
    """The reference composition: quantise(inverse(oracle.bm4d(forward(v), 1.0, stages)))."""
    c = _consts(params)
    return inverse(oracle.bm4d(forward(vol_u16, c), 1.0, stages=stages), c, inverse_kind)


def denoise_chunked(oracle, vol_u16, params, chunk, halo, inverse_kind="closed_form", stages=2, core=None):
    """The same composition on every truncated padded chunk (oracle.padded_chunks); only the cores are written."""
    c = _consts(params)
    vol = np.ascontiguousarray(vol_u16, dtype=np.uint16)
    zc0, zc1 = (0, vol.shape[0]) if core is None else core
    out = np.zeros((zc1 - zc0,) + vol.shape[1:], dtype=np.uint16)
    for sl, front, padded in oracle.padded_chunks(vol, chunk, halo, core):
        den = denoise(oracle, padded, c, inverse_kind, stages)
        inner = tuple(slice(f, f + (s.stop - s.start)) for f, s in zip(front, sl))
        out[(slice(sl[0].start - zc0, sl[0].stop - zc0),) + sl[1:]] = den[inner]
    return out
