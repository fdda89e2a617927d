"""The backward kernels of the BM4DNet stage's NDHWC layers (csrc/nn_grad_kernels.hip) against the fp64
restatement tests/nn_grad_pyref.py, with the framework's own fp32 CUDA backward measured by the same yardstick.

Yardstick (GroupNorm, up-sampling): ``max |got - ref| / S``, S = the reference evaluated on the absolute values
of its summands.  The kernel passes when its measure is <= 4 x the framework's (both are fp32 evaluations that
differ in summation order and in where they round) or <= 16 * 2^-24 (for inputs on which the framework happens
to be exact).  Both measures are printed.  The max-pool gradient places values: ``array_equal``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_grad_cases as cases
import nn_grad_pyref as ref
import nn_pyref
from aind_exaspim_image_compression import _native, inference

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
FLOOR = 16 * U


def dev(a):
    """fp32 [b, d, h, w, c] array -> CUDA tensor with that memory."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dev_ncdhw(a, grad=False):
    """The same values as a contiguous NCDHW CUDA tensor: the framework's own layout."""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a, dtype=np.float32), -1, 1))).cuda() \
        .requires_grad_(grad)


def host_ndhwc(t):
    return np.moveaxis(t.detach().cpu().numpy(), 1, -1)


def measure(got, want, s, kernel=True):
    """max |got - want| / S.  Where S == 0 every summand is 0 and so is the result: required of the kernel
    exactly (the framework's value there is its own business and is left out of its measure)."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    assert not kernel or np.all(err[s == 0] == 0)
    return float((err[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0


def judge(what, ours, theirs):
    print(f"{what}: kernel {ours / U:.3f} u, framework {theirs / U:.3f} u (u = 2^-24)")
    assert ours <= max(4 * theirs, FLOOR), (what, ours / U, theirs / U)


def stream():
    return torch.cuda.current_stream().cuda_stream


def gn_forward(ctx, x_dev, groups, gamma, beta, slope):
    b, c = x_dev.shape[0], x_dev.shape[-1]
    spatial = x_dev.numel() // (b * c)
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(b, spatial, c, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x_dev)
    stats = torch.empty((b, groups, 2), dtype=torch.float32, device="cuda")
    ctx.groupnorm_lrelu_ndhwc_train(stream(), x_dev, y, b, spatial, c, groups, gamma, beta, 1e-5, slope, ws, need,
                                    stats)
    return y, stats


def gn_backward(ctx, x_dev, y, dy_dev, dx, groups, gamma, stats, slope, affine_grads=True):
    b, c = x_dev.shape[0], x_dev.shape[-1]
    spatial = x_dev.numel() // (b * c)
    need = int(_native.lib().exabm4d_groupnorm_lrelu_bwd_workspace_bytes(b, spatial, c, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dg = torch.full((c,), np.nan, device="cuda") if affine_grads else None
    db = torch.full((c,), np.nan, device="cuda") if affine_grads else None
    ctx.groupnorm_lrelu_bwd_ndhwc(stream(), x_dev, y, dy_dev, dx, b, spatial, c, groups, gamma, stats, slope, dg, db,
                                  ws, need)
    return dg, db


def run_gn_case(ctx, shape, groups, slope, seed, affine=True, negative_gamma=False):
    x, dy, gamma, beta = cases.gn_case(shape, groups, slope, seed, affine, negative_gamma)
    # before any GPU call: no pre-activation within KINK of the kink (slope 1 has none)
    assert slope == 1.0 or cases.kink_free(x, groups, gamma, beta)
    r = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    x_dev, dy_dev = dev(x), dev(dy)
    g_dev = dev(gamma) if affine else None
    b_dev = dev(beta) if affine else None
    y, stats = gn_forward(ctx, x_dev, groups, g_dev, b_dev, slope)
    dx = torch.full_like(x_dev, np.nan)
    dg, db = gn_backward(ctx, x_dev, y, dy_dev, dx, groups, g_dev, stats, slope, affine)
    # the framework, fp32 CUDA, same inputs
    xt = dev_ncdhw(x, grad=True)
    wt = g_dev.clone().requires_grad_(True) if affine else None
    bt = b_dev.clone().requires_grad_(True) if affine else None
    F.leaky_relu(F.group_norm(xt, groups, wt, bt, 1e-5), slope).backward(dev_ncdhw(dy))
    tag = f"gn {shape} G={groups} slope={slope}"
    judge(tag + " dx", measure(dx.cpu().numpy(), r["dx"], r["S_dx"]),
          measure(host_ndhwc(xt.grad), r["dx"], r["S_dx"], kernel=False))
    if affine:
        judge(tag + " dgamma", measure(dg.cpu().numpy(), r["dgamma"], r["S_dgamma"]),
              measure(wt.grad.cpu().numpy(), r["dgamma"], r["S_dgamma"], kernel=False))
        judge(tag + " dbeta", measure(db.cpu().numpy(), r["dbeta"], r["S_dbeta"]),
              measure(bt.grad.cpu().numpy(), r["dbeta"], r["S_dbeta"], kernel=False))
    return x_dev, y, dy_dev, g_dev, stats, dx, dg, db


@pytest.mark.parametrize("slope", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("shape,groups", cases.GN_CASES)
def test_groupnorm_lrelu_backward(ctx, shape, groups, slope):
    x_dev, y, dy_dev, g_dev, stats, dx, dg, db = run_gn_case(ctx, shape, groups, slope, seed=21)
    # a second call on the same inputs: the same bits
    dx2 = torch.full_like(dx, np.nan)
    dg2, db2 = gn_backward(ctx, x_dev, y, dy_dev, dx2, groups, g_dev, stats, slope)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("shape,groups", [((2, 3, 5, 7, 32), 8), ((5, 2, 3, 2, 8), 2)])
def test_groupnorm_backward_negative_gamma_and_non_affine(ctx, shape, groups):
    run_gn_case(ctx, shape, groups, 0.01, seed=22, negative_gamma=True)
    run_gn_case(ctx, shape, groups, 0.2, seed=23, affine=False)


def test_groupnorm_backward_writes_only_its_view(ctx):
    shape, groups, slope = (2, 8, 8, 8, 32), 8, 0.01
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    x, dy, gamma, beta = cases.gn_case(shape, groups, slope, seed=24)
    assert cases.kink_free(x, groups, gamma, beta)
    x_dev, dy_dev, g_dev = dev(x), dev(dy), dev(gamma)
    y, stats = gn_forward(ctx, x_dev, groups, g_dev, dev(beta), slope)
    keep = [t.clone() for t in (x_dev, y, dy_dev, g_dev, stats)]
    buf = torch.full((pre + n + post,), -7.25, dtype=torch.float32, device="cuda")
    gn_backward(ctx, x_dev, y, dy_dev, buf[pre:pre + n].view(shape), groups, g_dev, stats, slope)
    host = buf.cpu().numpy()
    assert np.all(host[:pre] == -7.25) and np.all(host[pre + n:] == -7.25)
    r = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    assert measure(host[pre:pre + n].reshape(shape), r["dx"], r["S_dx"]) <= 64 * U
    for t, k in zip((x_dev, y, dy_dev, g_dev, stats), keep):
        assert torch.equal(t, k)                        # the inputs are read only


def test_forward_statistics_are_the_forwards_own(ctx):
    """The training entry writes y as the inference entry does (same kernels) plus (mean, rstd) in fp32."""
    shape, groups = (2, 3, 5, 7, 32), 8
    x, _, gamma, beta = cases.gn_case(shape, groups, 0.01, seed=25)
    x_dev, g_dev, b_dev = dev(x), dev(gamma), dev(beta)
    y, stats = gn_forward(ctx, x_dev, groups, g_dev, b_dev, 0.01)
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(2, 105, 32, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y0 = torch.empty_like(x_dev)
    ctx.groupnorm_lrelu_ndhwc(stream(), x_dev, y0, 2, 105, 32, groups, g_dev, b_dev, 1e-5, 0.01, ws, need)
    assert torch.equal(y, y0)
    mean, var = nn_pyref.group_norm_parts(x, groups)[:2]
    got = stats.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got[..., 0], mean, rtol=0, atol=4 * U * np.abs(x).max())
    np.testing.assert_allclose(got[..., 1], 1 / np.sqrt(var + 1e-5), rtol=4 * U)


@pytest.mark.parametrize("slope", [0.0, -0.1])
def test_slope_not_positive_is_unsupported_and_the_module_falls_back(ctx, slope):
    shape, groups = (1, 2, 2, 2, 32), 8
    x_dev = dev(np.random.default_rng(26).standard_normal(shape))
    lib = _native.lib()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    stats = torch.zeros((1, groups, 2), device="cuda")
    y = torch.empty_like(x_dev)
    p = lambda t: None if t is None else int(t.data_ptr())  # noqa: E731
    assert lib.exabm4d_groupnorm_lrelu_ndhwc_train_dev(ctx.handle, stream(), p(x_dev), p(y), 1, 8, 32, groups, None,
                                                       None, 1e-5, slope, p(ws), ws.numel(), p(stats)) == -2
    assert lib.exabm4d_groupnorm_lrelu_bwd_ndhwc_dev(ctx.handle, stream(), p(x_dev), p(y), p(x_dev), p(y), 1, 8, 32,
                                                     groups, None, p(stats), slope, None, None, p(ws),
                                                     ws.numel()) == -2
    mod = inference.FusedGroupNormLeakyReLU(torch.nn.GroupNorm(groups, 32).cuda(), torch.nn.LeakyReLU(slope),
                                            inplace=False, trainable=True)
    xin = x_dev.permute(0, 4, 1, 2, 3).requires_grad_(True)
    with torch.enable_grad():
        out = mod(xin)
    assert "LeakyRelu" in type(out.grad_fn).__name__
    mod.act = torch.nn.LeakyReLU(0.01)
    with torch.enable_grad():
        assert type(mod(xin).grad_fn).__name__ == "_GroupNormLeakyReLUFnBackward"


# ---- MaxPool3d(2) backward ---------------------------------------------------------------------------------
SENTINEL = -7.25


def pool_backward(ctx, x, dy):
    b, d, h, w, c = x.shape
    dx = torch.full(x.shape, SENTINEL, dtype=torch.float32, device="cuda")
    ctx.maxpool2_bwd_ndhwc(stream(), dev(x), dev(dy), dx, b, d, h, w, c)
    return dx.cpu().numpy()


def torch_pool_backward(x, dy):
    xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 1))).requires_grad_(True)
    F.max_pool3d(xt, 2).backward(torch.from_numpy(np.ascontiguousarray(np.moveaxis(dy, -1, 1))))
    return np.moveaxis(xt.grad.numpy(), 1, -1)


def pool_check(ctx, x, seed):
    b, d, h, w, c = x.shape
    dy = np.random.default_rng(seed).standard_normal((b, d // 2, h // 2, w // 2, c)).astype(np.float32)
    dy[dy == 0] = 1.0
    got = pool_backward(ctx, x, dy)
    want = torch_pool_backward(x, dy)
    assert np.array_equal(got, want)
    assert np.array_equal(got, ref.maxpool2_backward(x, dy))
    # the trailing voxels of odd extents: exactly 0 (the buffer held a sentinel)
    for axis, n in ((1, d), (2, h), (3, w)):
        if n % 2:
            assert np.all(np.take(got, n - 1, axis=axis) == 0)
    assert np.count_nonzero(got) == dy.size


@pytest.mark.parametrize("shape", cases.POOL_SHAPES)
def test_maxpool_backward(ctx, shape):
    pool_check(ctx, np.random.default_rng(31).standard_normal(shape).astype(np.float32), 32)


def test_maxpool_backward_ties_and_signed_zeros(ctx):
    pool_check(ctx, cases.pool_tie_input((2, 5, 6, 7, 8), 33), 34)


def test_maxpool_backward_nans(ctx):
    pool_check(ctx, cases.pool_nan_input(35), 36)


# ---- trilinear x2 up-sampling backward --------------------------------------------------------------------
def up_check(ctx, shape):
    """The up-sampling gradient at input ``shape``: run to run, ``judge`` against fp64, and the adjoint identity."""
    b, d, h, w, c = shape
    rng = np.random.default_rng(41)
    dy = rng.standard_normal((b, 2 * d, 2 * h, 2 * w, c)).astype(np.float32)
    want, s = ref.upsample2_trilinear_backward(dy)
    dy_dev = dev(dy)
    dx = torch.full(shape, np.nan, dtype=torch.float32, device="cuda")
    ctx.upsample2_trilinear_bwd_ndhwc(stream(), dy_dev, dx, b, d, h, w, c)
    dx2 = torch.full(shape, np.nan, dtype=torch.float32, device="cuda")
    ctx.upsample2_trilinear_bwd_ndhwc(stream(), dy_dev, dx2, b, d, h, w, c)
    assert torch.equal(dx, dx2)
    xt = torch.zeros((b, c, d, h, w), device="cuda", requires_grad=True)
    F.interpolate(xt, scale_factor=2, mode="trilinear", align_corners=True).backward(dev_ncdhw(dy))
    judge(f"up {shape} dx", measure(dx.cpu().numpy(), want, s), measure(host_ndhwc(xt.grad), want, s, kernel=False))
    # <up(x), dy> == <x, up^T(dy)>, both from the GPU's results, in fp64
    x = rng.standard_normal(shape).astype(np.float32)
    up = torch.empty((b, 2 * d, 2 * h, 2 * w, c), dtype=torch.float32, device="cuda")
    ctx.upsample2_trilinear_ndhwc(stream(), dev(x), up, b, d, h, w, c)
    lhs_terms = up.cpu().numpy().astype(np.float64) * dy
    rhs_terms = x.astype(np.float64) * dx.cpu().numpy().astype(np.float64)
    lhs, rhs = lhs_terms.sum(), rhs_terms.sum()
    bound = 8 * U * (np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    print(f"up {shape} adjoint: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("shape", cases.UP_SHAPES)
def test_upsample_backward(ctx, shape):
    up_check(ctx, shape)


def test_resample_modules_run_the_native_functions(ctx):
    x = dev(np.random.default_rng(42).standard_normal((1, 5, 4, 6, 8))).permute(0, 4, 1, 2, 3).requires_grad_(True)
    pool = inference._ResampleNDHWC(torch.nn.MaxPool3d(2), trainable=True)
    up = inference._ResampleNDHWC(torch.nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
                                  trainable=True)
    with torch.enable_grad():
        y = up(pool(x))
    assert type(y.grad_fn).__name__ == "_Upsample2FnBackward"
    g = torch.randn_like(y)
    y.backward(g)
    xt = x.detach().contiguous().requires_grad_(True)
    F.interpolate(F.max_pool3d(xt, 2), scale_factor=2, mode="trilinear", align_corners=True).backward(g.contiguous())
    assert torch.allclose(x.grad, xt.grad, rtol=1e-5, atol=1e-5)
    assert torch.equal(x.grad == 0, xt.grad == 0)
