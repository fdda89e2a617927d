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


def test_conditional_reference_with_the_fp64_statistics_is_the_reference():
    """``stats`` computed in fp64 from x: every returned array has the bits of the unconditional reference."""
    shape, groups = (2, 3, 5, 7, 32), 8
    x, dy, gamma, beta = cases.gn_case(shape, groups, 0.2, seed=10, negative_gamma=True)
    mean, var = nn_pyref.group_norm_parts(x, groups)[:2]
    a = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, 0.2)
    b = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, 0.2, stats=(mean, 1.0 / np.sqrt(var + 1e-5)))
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
    # the extra outputs are what their names say
    cpg = 32 // groups
    assert a["m1"].shape == a["m2"].shape == a["mean"].shape == a["rstd"].shape == (2, groups)
    close(a["dgamma_b"].sum(axis=0), a["dgamma"], a["S_dgamma"])
    close(a["dbeta_b"].sum(axis=0), a["dbeta"], a["S_dbeta"])
    dz = dy.astype(np.float64) * np.where(a["z"] > 0, 1.0, 0.2)
    gdz = (gamma.astype(np.float64) * dz).reshape(2, -1, groups, cpg)
    np.testing.assert_allclose(a["m1"], gdz.mean(axis=(1, 3)), rtol=RTOL)
    np.testing.assert_allclose(a["m2"], (gdz * a["xh"].reshape(gdz.shape)).mean(axis=(1, 3)), rtol=RTOL, atol=1e-15)
    # other statistics give another answer, and the side of the kink stays the true z's
    c = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, 0.2, stats=(mean + 10.0, a["rstd"]))
    assert np.array_equal(c["z"], a["z"]) and np.array_equal(c["dbeta"], a["dbeta"])
    assert not np.allclose(c["dx"], a["dx"])


@pytest.mark.parametrize("kind", ["mean1000", "std1e-3", "constant", "spread"])
def test_groupnorm_backward_on_hostile_distributions(kind):
    """The reference against torch's CPU float64 autograd where the statistics amplify, at this file's criterion."""
    shape, groups, slope = (2, 3, 5, 7, 32), 8, 0.01
    x, dy, gamma, beta = cases.gn_case_kind(kind, shape, groups, slope, seed=11)
    xt = ncdhw(x, grad=True)
    w = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    F.leaky_relu(F.group_norm(xt, groups, w, b, 1e-5), slope).backward(ncdhw(dy))
    r = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    cpg = shape[-1] // groups
    close(r["dx"], ndhwc(xt.grad), r["S_dx"])
    cond = np.abs(dy).sum(axis=(0, 1, 2, 3)) * np.repeat((np.abs(r["mean"]) * r["rstd"]).max(axis=0), cpg)
    close(r["dgamma"], w.grad.numpy(), r["S_dgamma"] + cond)
    close(r["dbeta"], b.grad.numpy(), r["S_dbeta"])


@pytest.mark.parametrize("slope", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("kind", cases.GN_KINDS)
def test_gn_case_kind_ends_kink_free(kind, slope):
    """The builder asserts |z| >= max(KINK, 2 E) itself; here also from outside (KINK >= 2 E everywhere but on
    ``constant``: its E is 6e-4, its smallest |z| 0.1), and that the nudging leaves the distribution what its name
    says (at most a few elements move, by 1/32 of a deviation each round)."""
    shape, groups = (2, 16, 16, 16, 32), 8
    x, dy, gamma, beta = cases.gn_case_kind(kind, shape, groups, slope, seed=12)
    assert x.dtype == dy.dtype == gamma.dtype == beta.dtype == np.float32
    assert cases.kink_free(x, groups, gamma, beta)
    assert (gamma < 0).any() and (gamma > 0).any()
    z, E = cases.gn_preact_bound(x, groups, gamma, beta)
    assert np.all(np.abs(z) >= 2 * E) and (kind == "constant" or cases.KINK >= 2 * E.max())
    moved = x != cases.gn_inputs(kind, shape, groups, 12)
    assert np.count_nonzero(moved) <= x.size // 100
    x2 = cases.gn_case_kind(kind, shape, groups, 0.5, seed=12)[0]
    assert np.array_equal(x, x2)                              # the slopes of a case share their x


def test_gn_case_kind_mixed_batch_and_dead_channels():
    shape, groups = (3, 2, 3, 4, 16), 4
    x = cases.gn_case_kind(["constant", "mean1000", "std1e-3"], shape, groups, 0.01, seed=13)[0]
    assert np.all(x[0] == np.float32(5.3)) and abs(x[1].mean() - 1000) < 1 and abs(x[2].mean() - 1) < 1e-3
    gamma, beta = np.ones(16, np.float32), np.full(16, 0.25, np.float32)
    gamma[[2, 5]] = 0
    beta[2], beta[5] = 0.0, -0.0
    x, _, g2, b2 = cases.gn_case_kind("today", shape, groups, 0.01, seed=14, gamma=gamma, beta=beta, exact_zero=[2, 5])
    assert g2 is gamma and b2 is beta
    z = nn_pyref.group_norm_parts(x, groups, gamma, beta)[3]
    assert np.all(z[..., [2, 5]] == 0) and np.all(np.abs(np.delete(z, [2, 5], axis=-1)) >= cases.KINK)
    with pytest.raises(AssertionError):                        # a live channel at the kink is not excepted
        cases.gn_case_kind("constant", shape, groups, 0.01, seed=14, gamma=gamma, beta=np.zeros(16, np.float32),
                           exact_zero=[2, 5])


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
