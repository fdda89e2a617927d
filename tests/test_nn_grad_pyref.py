"""tests/nn_grad_pyref.py (the fp64 yardstick of the training kernels) against torch's CPU float64 autograd of
the framework's own modules, at the shapes the GPU tests use (CPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_grad_cases as cases
import nn_grad_pyref as ref
import nn_pyref

RTOL = 1e-12


def ncdhw(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a, dtype=np.float64), -1, 1))).requires_grad_(
        kw.get("grad", False))


def ndhwc(t):
    return np.moveaxis(t.detach().numpy(), 1, -1)


def close(got, want, scale):
    """Equality to fp64 rounding: rtol 1e-12, measured against the summands' magnitude where the result is a
    sum that cancels (``scale``, the S of nn_grad_pyref)."""
    assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), scale))


@pytest.mark.parametrize("slope", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("shape,groups", cases.GN_CASES)
def test_groupnorm_lrelu_backward(shape, groups, slope):
    x, dy, gamma, beta = cases.gn_case(shape, groups, slope, seed=1)
    assert slope == 1.0 or cases.kink_free(x, groups, gamma, beta)
    xt = ncdhw(x, grad=True)
    w = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    F.leaky_relu(F.group_norm(xt, groups, w, b, 1e-5), slope).backward(ncdhw(dy))
    r = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    close(r["dx"], ndhwc(xt.grad), r["S_dx"])
    # xh = x rstd - mean rstd is itself a difference that cancels (completely on the constant one-voxel input,
    # where the reference has xh = 0 and torch a rounding residue): dgamma's scale carries those two terms
    mean, var = nn_pyref.group_norm_parts(x, groups)[:2]
    cond = np.abs(dy).sum(axis=(0, 1, 2, 3)) * np.repeat((np.abs(mean) / np.sqrt(var + 1e-5)).max(axis=0),
                                                          shape[-1] // groups)
    close(r["dgamma"], w.grad.numpy(), r["S_dgamma"] + cond)
    close(r["dbeta"], b.grad.numpy(), r["S_dbeta"])


def test_groupnorm_backward_non_affine_and_negative_gamma():
    shape, groups = (2, 3, 5, 7, 32), 8
    x, dy, gamma, beta = cases.gn_case(shape, groups, 0.2, seed=2, negative_gamma=True)
    assert (gamma < 0).any()
    xt = ncdhw(x, grad=True)
    F.leaky_relu(F.group_norm(xt, groups, torch.from_numpy(gamma.astype(np.float64)),
                              torch.from_numpy(beta.astype(np.float64)), 1e-5), 0.2).backward(ncdhw(dy))
    r = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, 0.2)
    close(r["dx"], ndhwc(xt.grad), r["S_dx"])
    x, dy, _, _ = cases.gn_case(shape, groups, 0.01, seed=3, affine=False)
    xt = ncdhw(x, grad=True)
    F.leaky_relu(F.group_norm(xt, groups, None, None, 1e-5), 0.01).backward(ncdhw(dy))
    r = ref.group_norm_lrelu_backward(x, dy, groups, None, None, 1e-5, 0.01)
    close(r["dx"], ndhwc(xt.grad), r["S_dx"])


def torch_pool_backward(x, dy):
    xt = ncdhw(x, grad=True)
    F.max_pool3d(xt, 2).backward(ncdhw(dy))
    return ndhwc(xt.grad)


@pytest.mark.parametrize("shape", cases.POOL_SHAPES)
def test_maxpool_backward(shape):
    rng = np.random.default_rng(4)
    x = rng.standard_normal(shape).astype(np.float32)
    dy = rng.standard_normal((shape[0], shape[1] // 2, shape[2] // 2, shape[3] // 2, shape[4]))
    assert np.array_equal(ref.maxpool2_backward(x, dy), torch_pool_backward(x, dy))


def test_maxpool_backward_ties_signed_zeros_and_nans():
    rng = np.random.default_rng(5)
    x = cases.pool_tie_input((2, 4, 6, 5, 8), 6)
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    dy = rng.standard_normal((2, 2, 3, 2, 8))
    assert np.array_equal(ref.maxpool2_backward(x, dy), torch_pool_backward(x, dy))
    x = np.zeros((1, 2, 2, 2, 4), dtype=np.float32)              # one window, all equal: the first position
    dx = ref.maxpool2_backward(x, np.ones((1, 1, 1, 1, 4)))
    assert dx[0, 0, 0, 0].tolist() == [1.0] * 4 and dx.sum() == 4.0
    x = cases.pool_nan_input(7)
    dy = rng.standard_normal((1, 2, 2, 3, 4))
    assert np.array_equal(ref.maxpool2_backward(x, dy), torch_pool_backward(x, dy))


@pytest.mark.parametrize("shape", cases.UP_SHAPES)
def test_upsample_backward(shape):
    b, d, h, w, c = shape
    dy = np.random.default_rng(8).standard_normal((b, 2 * d, 2 * h, 2 * w, c))
    xt = torch.zeros((b, c, d, h, w), dtype=torch.float64, requires_grad=True)
    F.interpolate(xt, scale_factor=2, mode="trilinear", align_corners=True).backward(ncdhw(dy))
    dx, s = ref.upsample2_trilinear_backward(dy)
    close(dx, ndhwc(xt.grad), s)


@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("fg_weight", [0.0, 20.0])
def test_charbonnier_loss_and_gradient(n, fg_weight):
    rng = np.random.default_rng(9)
    pred, target = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    mask = (rng.random(n) < 0.3).astype(np.float32)
    p = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    t, m = torch.from_numpy(target.astype(np.float64)), torch.from_numpy(mask.astype(np.float64))
    loss = ((1.0 + fg_weight * m) * torch.sqrt((p - t) * (p - t) + 1e-3 * 1e-3)).mean()
    loss.backward()
    assert abs(ref.charbonnier_loss(pred, target, mask, fg_weight) - float(loss.detach())) <= RTOL * float(loss.detach())
    np.testing.assert_allclose(ref.charbonnier_loss_backward(pred, target, mask, fg_weight), p.grad.numpy(),
                               rtol=RTOL, atol=0)
