"""Plain float64 restatement of the BM4DNet stage's three NDHWC kernels (csrc/nn_kernels.hip), written from
the definitions of the framework's operations and not from the kernels: GroupNorm (+ the preceding
convolution's bias) + LeakyReLU, MaxPool3d(2), and trilinear x2 up-sampling with ``align_corners=True``.

Arrays are channels-last: ``x[b, d, h, w, c]`` (or ``x[b, s, c]`` with the spatial axes flattened for the
GroupNorm).  Small and medium tensors only; everything is vectorised numpy.  The reference itself is checked
against torch's CPU float64 functional ops in ``test_nn_pyref.py``."""
import numpy as np


def group_norm_parts(x, groups, gamma=None, beta=None, eps=1e-5, cbias=None):
    """The fp64 quantities of ``GroupNorm(groups, C)(x + cbias)``: ``mean[b, g]``, biased ``var[b, g]``,
    the per-(sample, channel) scale ``a[b, c] = gamma[c] / sqrt(var + eps)`` and the pre-activation
    ``z = a (x + cbias - mean) + beta`` (shape of ``x``).  Statistics are two-pass in fp64.  A group holding
    any non-finite value has NaN statistics, so all of it comes out NaN."""
    x = np.asarray(x)
    B, C = x.shape[0], x.shape[-1]
    assert C % groups == 0
    v = x.astype(np.float64).reshape(B, -1, C)
    if cbias is not None:
        v = v + np.asarray(cbias, dtype=np.float64)
    vg = v.reshape(B, v.shape[1], groups, C // groups)
    finite = np.isfinite(vg).all(axis=(1, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.where(finite, vg.mean(axis=(1, 3)), np.nan)
        var = np.where(finite, ((vg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3)), np.nan)
        g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
        b = np.zeros(C) if beta is None else np.asarray(beta, dtype=np.float64)
        rstd = 1.0 / np.sqrt(var + eps)                                    # [B, G]
        a = np.repeat(rstd, C // groups, axis=1) * g                        # [B, C]
        mean_c = np.repeat(mean, C // groups, axis=1)                       # [B, C]
        z = (v - mean_c[:, None, :]) * a[:, None, :] + b
    return mean, var, a, z.reshape(x.shape)


def leaky_relu(z, slope):
    """``z if z > 0 else z * slope`` (NaN stays NaN, -0 stays -0)."""
    with np.errstate(invalid="ignore"):
        return np.where(z > 0, z, z * slope)


def group_norm_lrelu(x, groups, gamma=None, beta=None, eps=1e-5, slope=0.01, cbias=None):
    """``leaky_relu(group_norm(x + cbias, groups, gamma, beta, eps), slope)`` in fp64 on a channels-last
    array; ``gamma`` / ``beta`` None: the affine=False module."""
    return leaky_relu(group_norm_parts(x, groups, gamma, beta, eps, cbias)[3], slope)


def maxpool2(x):
    """MaxPool3d(2) on ``x[b, d, h, w, c]``: odd extents are floored; the eight window positions are
    visited in (d, h, w) raster order and a position replaces the running maximum when it is larger or NaN --
    so the first of equal values wins (which fixes the sign of a -0 / +0 tie) and a NaN wins.  Keeps the dtype
    (it selects, it does not compute)."""
    x = np.asarray(x)
    B, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    v = x[:, :2 * OD, :2 * OH, :2 * OW, :].reshape(B, OD, 2, OH, 2, OW, 2, C)
    m = v[:, :, 0, :, 0, :, 0, :].copy()
    for k in range(1, 8):
        kd, kh, kw = k >> 2, (k >> 1) & 1, k & 1
        c = v[:, :, kd, :, kh, :, kw, :]
        with np.errstate(invalid="ignore"):
            take = (c > m) | np.isnan(c)
        m = np.where(take, c, m)
    return m


def _up_axis(n_in):
    """Source indices and weights of one axis of the x2 align-corners interpolation: ``src = r * o`` with
    the exact ratio ``r = (in - 1) / (out - 1)`` in fp64 (0 for an output extent of 1), ``i0 = floor(src)``,
    ``i1 = min(i0 + 1, in - 1)``, weights ``(1 - lambda, lambda)``."""
    n_out = 2 * n_in
    r = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    src = r * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def upsample2_trilinear(x):
    """Upsample(scale_factor=2, mode="trilinear", align_corners=True) on ``x[b, d, h, w, c]`` in fp64:
    linear along w, then h, then d, each as ``w0 * a + w1 * c`` -- so a non-finite neighbour with weight 0
    still poisons the result (0 * inf = NaN), as in the framework."""
    x = np.asarray(x, dtype=np.float64)
    (d0, d1, dw0, dw1), (h0, h1, hw0, hw1), (w0, w1, ww0, ww1) = (_up_axis(n) for n in x.shape[1:4])
    with np.errstate(invalid="ignore", over="ignore"):
        t = ww0[:, None] * x[:, :, :, w0, :] + ww1[:, None] * x[:, :, :, w1, :]
        t = hw0[:, None, None] * t[:, :, h0] + hw1[:, None, None] * t[:, :, h1]
        return dw0[:, None, None, None] * t[:, d0] + dw1[:, None, None, None] * t[:, d1]
