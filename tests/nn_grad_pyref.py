"""Plain float64 restatement of the BM4DNet training kernels (csrc/nn_grad_kernels.hip), written from the
formulas and not from the kernels: the backward passes of GroupNorm + LeakyReLU, MaxPool3d(2) and trilinear x2
up-sampling (align_corners) on channels-last arrays ``[b, d, h, w, c]``, and the foreground-weighted Charbonnier
loss with its gradient.  Checked against torch's CPU float64 autograd in ``test_nn_grad_pyref.py``.

Where a result is a sum, the function also returns ``S``: the same expression evaluated on the absolute values of
its summands.  ``|got - ref| / S`` is then the error of an fp32 evaluation in units that do not blow up where
the summands cancel."""
import numpy as np

import nn_pyref


def group_norm_lrelu_backward(x, dy, groups, gamma=None, beta=None, eps=1e-5, slope=0.01, stats=None):
    """Gradients of ``y = leaky_relu(group_norm(x))``: a dict with ``dx`` (shape of x), ``dgamma``, ``dbeta``
    ([C]; the parameter gradients of the affine module whether or not gamma is given), their ``S_dx``,
    ``S_dgamma``, ``S_dbeta``, and the pre-activation ``z``.
      dz = dy (z > 0 ? 1 : slope)      xh = (x - mean) rstd
      dbeta = sum_{b,s} dz             dgamma = sum_{b,s} dz xh
      dx = rstd (gamma dz - m1 - xh m2), m1, m2 = means over a (sample, group) of gamma dz and gamma dz xh
    ``stats = (mean[b, g], rstd[b, g])``: the conditional reference -- these values stand in the formulas
    instead of the statistics of x (what a backward pass that is handed a forward's statistics should give, to
    fp64).  The side of the kink is the true fp64 z's either way.  Also returned, for bounds on how an error of
    the statistics propagates: ``mean``, ``rstd``, ``m1``, ``m2`` ([b, g], as used), ``xh`` (shape of x) and the
    per-sample summands ``dgamma_b``, ``dbeta_b`` ([b, C])."""
    x = np.asarray(x)
    B, C = x.shape[0], x.shape[-1]
    cpg = C // groups
    mean, var, _, z = nn_pyref.group_norm_parts(x, groups, gamma, beta, eps)
    rstd_g = 1.0 / np.sqrt(var + eps)
    if stats is not None:
        mean, rstd_g = (np.asarray(s, dtype=np.float64).reshape(B, groups) for s in stats)
    v = x.astype(np.float64).reshape(B, -1, C)
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float64)
    rstd = np.repeat(rstd_g, cpg, axis=1)[:, None, :]                            # [B, 1, C]
    xh = (v - np.repeat(mean, cpg, axis=1)[:, None, :]) * rstd
    dz = np.asarray(dy, dtype=np.float64).reshape(B, -1, C) * np.where(z.reshape(B, -1, C) > 0, 1.0, slope)

    def group_mean(t):                                                           # [B, S, C] -> [B, G]
        return t.reshape(B, t.shape[1], groups, cpg).mean(axis=(1, 3))

    def per_channel(m):                                                          # [B, G] -> [B, 1, C]
        return np.repeat(m, cpg, axis=1)[:, None, :]

    gdz = g * dz
    m1, m2 = group_mean(gdz), group_mean(gdz * xh)
    dx = rstd * (gdz - per_channel(m1) - xh * per_channel(m2))
    s_dx = rstd * (np.abs(gdz) + per_channel(group_mean(np.abs(gdz)))
                   + np.abs(xh) * per_channel(group_mean(np.abs(gdz * xh))))
    dgamma_b, dbeta_b = (dz * xh).sum(axis=1), dz.sum(axis=1)
    return {"dx": dx.reshape(x.shape), "S_dx": s_dx.reshape(x.shape),
            "dgamma": (dz * xh).sum(axis=(0, 1)), "S_dgamma": np.abs(dz * xh).sum(axis=(0, 1)),
            "dbeta": dz.sum(axis=(0, 1)), "S_dbeta": np.abs(dz).sum(axis=(0, 1)), "z": z,
            "mean": mean, "rstd": rstd_g, "m1": m1, "m2": m2, "xh": xh.reshape(x.shape),
            "dgamma_b": dgamma_b, "dbeta_b": dbeta_b}


def maxpool2_argmax(x):
    """Per window and channel the position 0..7 (``kd * 4 + kh * 2 + kw``) torch's max_pool3d selects: scan in
    (d, h, w) order, replace the running maximum when ``v > max`` or ``v`` is NaN."""
    x = np.asarray(x)
    B, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    v = x[:, :2 * OD, :2 * OH, :2 * OW, :].reshape(B, OD, 2, OH, 2, OW, 2, C)
    m = v[:, :, 0, :, 0, :, 0, :].copy()
    idx = np.zeros(m.shape, dtype=np.int64)
    for k in range(1, 8):
        c = v[:, :, k >> 2, :, (k >> 1) & 1, :, k & 1, :]
        with np.errstate(invalid="ignore"):
            take = (c > m) | np.isnan(c)
        m = np.where(take, c, m)
        idx = np.where(take, k, idx)
    return idx


def maxpool2_backward(x, dy):
    """``dx`` of MaxPool3d(2): ``dy`` at the selected position of each window, 0 at the other seven and on the
    trailing plane / row / column of an odd extent.  Keeps ``dy``'s dtype (it places, it does not compute)."""
    x, dy = np.asarray(x), np.asarray(dy)
    B, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    idx = maxpool2_argmax(x)
    dx = np.zeros(x.shape, dtype=dy.dtype)
    win = dx[:, :2 * OD, :2 * OH, :2 * OW, :].reshape(B, OD, 2, OH, 2, OW, 2, C)   # a view of dx
    for k in range(8):
        win[:, :, k >> 2, :, (k >> 1) & 1, :, k & 1, :] = np.where(idx == k, dy, 0)
    return dx


def _up_matrix(n_in):
    """``A[o, i]``: the weight of input i in output o along one axis (fp64 indices and weights of nn_pyref)."""
    i0, i1, w0, w1 = nn_pyref._up_axis(n_in)
    a = np.zeros((2 * n_in, n_in))
    o = np.arange(2 * n_in)
    np.add.at(a, (o, i0), w0)
    np.add.at(a, (o, i1), w1)
    return a


def upsample2_trilinear_backward(dy):
    """``(dx, S)`` of the x2 align-corners up-sampling: the transpose of ``nn_pyref.upsample2_trilinear`` applied
    to ``dy[b, 2d, 2h, 2w, c]``; S: the same on ``|dy|`` (the weights are not negative)."""
    dy = np.asarray(dy, dtype=np.float64)
    ad, ah, aw = (_up_matrix(n // 2) for n in dy.shape[1:4])

    def t(v):
        return np.einsum("bxyzc,xd,yh,zw->bdhwc", v, ad, ah, aw, optimize=True)

    return t(dy), t(np.abs(dy))


def charbonnier_loss(pred, target, mask, fg_weight=20.0, eps=1e-3):
    """``mean((1 + fg_weight m) sqrt((pred - target)^2 + eps^2))`` in fp64."""
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    w = 1.0 + fg_weight * np.asarray(mask, dtype=np.float64)
    return float((w * np.sqrt(d * d + eps * eps)).mean())


def charbonnier_loss_backward(pred, target, mask, fg_weight=20.0, eps=1e-3, grad=1.0):
    """``dL/dpred = grad (1 + fg_weight m) d / sqrt(d^2 + eps^2) / N``."""
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    w = 1.0 + fg_weight * np.asarray(mask, dtype=np.float64)
    return grad * w * d / np.sqrt(d * d + eps * eps) / d.size
