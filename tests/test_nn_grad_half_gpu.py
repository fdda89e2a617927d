"""The backward kernels of the BM4DNet stage's NDHWC layers in fp16 / bf16 storage (csrc/nn_grad_kernels.hip through
the ``*_dt_dev`` training entries).

The half instances widen their inputs exactly, evaluate the fp32 instance's expressions and round each output
once.  So on inputs that ARE half values:

  A. dgamma, dbeta are the bits the fp32 entry gives on the widened inputs, and dx is that entry's dx ``.to(T)``;
  B. against the fp64 restatement ``nn_grad_pyref`` of the widened inputs,
     ``|dx - want| <= ulp_T(want) + max(4 m32, 16 * 2^-24) S_dx`` elementwise, where m32 is the fp32 entry's own
     measure ``max |dx32 - want| / S_dx`` on these inputs (factor and floor as in ``test_nn_grad_gpu``).

Printed per case: m32, the half kernel's excess over the bound of B (<= 1 passes) and, not asserted, the same
figure for the framework's autocast evaluation (``F.group_norm`` runs in fp32 under autocast; its input gradient
cast to T).  The max-pool gradient places values: ``array_equal``.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_grad_cases as cases
import nn_grad_pyref as ref
import nn_pyref
from test_nn_half_gpu import DTYPES, to_dev, ulp, widen

from aind_exaspim_image_compression import _native, inference

gpu = pytest.mark.gpu
U = 2.0 ** -24
FLOOR = 16 * U
SENTINEL = -7.25
_inputs = {}


def round_to(a, dtype):
    """fp32 array -> the nearest values of ``dtype`` (ties to even), as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def half_gn_case(name, shape, groups, slope, seed, affine=True, negative_gamma=False):
    """``cases.gn_case`` with x and dy rounded to the storage type, and the kink nudging repeated on the rounded x:
    every nudge is re-rounded, and where 0.03125 is below the type's spacing at max |x| (it would round away) the
    step is two spacings.  Returns fp32 arrays holding half values, computed once per case and never modified; the
    last element tells whether the loop ended with every |z| >= KINK."""
    key = (name, shape, groups, slope, seed, affine, negative_gamma)
    if key not in _inputs:
        dtype = DTYPES[name]
        x, dy, gamma, beta = cases.gn_case(shape, groups, slope, seed, affine, negative_gamma)
        x, dy = round_to(x, dtype), round_to(dy, dtype)
        done = slope == 1.0
        if not done:
            spacing = float(ulp(np.abs(x).max(), dtype))
            step = np.float32(0.03125 if 0.03125 >= spacing else 2 * spacing)
            for _ in range(100):
                bad = np.abs(nn_pyref.group_norm_parts(x, groups, gamma, beta, 1e-5)[3]) < cases.KINK
                if not bad.any():
                    done = True
                    break
                x[bad] += step
                x = round_to(x, dtype)
        _inputs[key] = (x, dy, gamma, beta, done)
    return _inputs[key]


GN_RUNS = ([(s, g, slope, 21, True, False) for s, g in cases.GN_CASES for slope in (0.01, 1.0)]
           + [(s, g, 0.01, 22, True, True) for s, g in [((2, 3, 5, 7, 32), 8), ((5, 2, 3, 2, 8), 2)]]
           + [(s, g, 0.2, 23, False, False) for s, g in [((2, 3, 5, 7, 32), 8), ((5, 2, 3, 2, 8), 2)]])


@pytest.mark.parametrize("name", DTYPES)
def test_nudging_ends_kink_free_for_every_case(name):
    """No GPU: the nudging loop on the rounded inputs terminates for every case of this file, in both types."""
    for shape, groups, slope, seed, affine, neg in GN_RUNS + [((2, 8, 8, 8, 32), 8, 0.01, 24, True, False)]:
        x, _, gamma, beta, done = half_gn_case(name, shape, groups, slope, seed, affine, neg)
        assert done, (name, shape, slope)
        assert slope == 1.0 or cases.kink_free(x, groups, gamma, beta)
        assert np.array_equal(x, round_to(x, DTYPES[name]))


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dims(t):
    """(batch, spatial, channels) of a [b, c, d, h, w] NDHWC tensor."""
    b, c = int(t.shape[0]), int(t.shape[1])
    return b, t.numel() // (b * c), c


def gn_forward(ctx, x, groups, gamma, beta, slope, code):
    b, spatial, c = dims(x)
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(b, spatial, c, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)                                # preserves the NDHWC strides
    stats = torch.empty((b, groups, 2), dtype=torch.float32, device="cuda")
    ctx.groupnorm_lrelu_ndhwc_train(stream(), x, y, b, spatial, c, groups, gamma, beta, 1e-5, slope, ws, need, stats,
                                    dtype=code)
    return y, stats


def gn_backward(ctx, x, y, dy, dx, groups, gamma, stats, slope, code, affine_grads=True):
    b, spatial, c = dims(x)
    need = int(_native.lib().exabm4d_groupnorm_lrelu_bwd_workspace_bytes(b, spatial, c, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dg = torch.full((c,), np.nan, device="cuda") if affine_grads else None
    db = torch.full((c,), np.nan, device="cuda") if affine_grads else None
    ctx.groupnorm_lrelu_bwd_ndhwc(stream(), x, y, dy, dx, b, spatial, c, groups, gamma, stats, slope, dg, db, ws, need,
                                  dtype=code)
    return dg, db


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def bound_b(want, s, got32, dtype):
    """The elementwise bound of condition B and m32."""
    err32 = np.abs(got32.astype(np.float64) - want)
    assert np.all(err32[s == 0] == 0)
    m32 = float((err32[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0
    return ulp(want, dtype) + max(4 * m32, FLOOR) * s, m32


@gpu
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape,groups,slope,seed,affine,neg", GN_RUNS)
def test_groupnorm_lrelu_backward(ctx, name, shape, groups, slope, seed, affine, neg):
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    x, dy, gamma, beta, done = half_gn_case(name, shape, groups, slope, seed, affine, neg)
    # before any GPU call: no pre-activation of the rounded x within KINK of the kink (slope 1 has none)
    assert done and (slope == 1.0 or cases.kink_free(x, groups, gamma, beta))
    want = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    x_t, dy_t = to_dev(x, dtype), to_dev(dy, dtype)
    assert np.array_equal(widen(x_t), x) and np.array_equal(widen(dy_t), dy)
    g_dev, b_dev = f32_dev(gamma), f32_dev(beta)
    y_t, stats = gn_forward(ctx, x_t, groups, g_dev, b_dev, slope, code)
    dx_t = torch.full_like(x_t, np.nan)
    dg, db = gn_backward(ctx, x_t, y_t, dy_t, dx_t, groups, g_dev, stats, slope, code, affine)
    # A: the fp32 entry on the widened x, y, dy with the same (mean, rstd)
    x32, y32, dy32 = x_t.float(), y_t.float(), dy_t.float()
    assert x32.is_contiguous(memory_format=torch.channels_last_3d)
    dx32 = torch.full_like(x32, np.nan)
    dg32, db32 = gn_backward(ctx, x32, y32, dy32, dx32, groups, g_dev, stats, slope, _native.DTYPE_F32, affine)
    assert torch.equal(bits(dx_t), bits(dx32.to(dtype)))
    if affine:
        assert torch.equal(bits(dg), bits(dg32)) and torch.equal(bits(db), bits(db32))
    # B: against fp64
    got = widen(dx_t)
    assert np.isfinite(got).all()
    bound, m32 = bound_b(want["dx"], want["S_dx"], widen(dx32), dtype)
    over = float((np.abs(got.astype(np.float64) - want["dx"]) / bound).max())
    # the framework under autocast: group_norm in fp32 on the widened x, the gradient cast to T
    xt = x32.detach().contiguous().requires_grad_(True)
    F.leaky_relu(F.group_norm(xt, groups, g_dev, b_dev, 1e-5), slope).backward(dy32.contiguous())
    fw = widen(xt.grad.to(dtype))
    over_fw = float((np.abs(fw.astype(np.float64) - want["dx"]) / bound).max())
    print(f"gn {name} {shape} G={groups} slope={slope} affine={affine} neg={neg}: m32 {m32 / U:.3f} u, "
          f"half kernel {over:.3f} x bound, framework autocast {over_fw:.3f} x bound")
    assert over <= 1.0, (name, shape, slope, over)
    # a second launch: the same bytes
    dx2 = torch.full_like(x_t, np.nan)
    dg2, db2 = gn_backward(ctx, x_t, y_t, dy_t, dx2, groups, g_dev, stats, slope, code, affine)
    assert torch.equal(bits(dx_t), bits(dx2))
    if affine:
        assert torch.equal(bits(dg), bits(dg2)) and torch.equal(bits(db), bits(db2))


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_training_forward_is_the_half_forward_plus_statistics(ctx, name):
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    shape, groups = (2, 3, 5, 7, 32), 8
    x, _, gamma, beta, _ = half_gn_case(name, shape, groups, 0.01, 25)
    x_t, g_dev, b_dev = to_dev(x, dtype), f32_dev(gamma), f32_dev(beta)
    y, stats = gn_forward(ctx, x_t, groups, g_dev, b_dev, 0.01, code)
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(2, 105, 32, groups))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y0 = torch.empty_like(x_t)
    ctx.groupnorm_lrelu_ndhwc(stream(), x_t, y0, 2, 105, 32, groups, g_dev, b_dev, 1e-5, 0.01, ws, need, dtype=code)
    assert y.dtype == dtype and torch.equal(bits(y), bits(y0))
    mean, var = nn_pyref.group_norm_parts(x, groups)[:2]
    got = stats.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got[..., 0], mean, rtol=0, atol=4 * U * np.abs(x).max())
    np.testing.assert_allclose(got[..., 1], 1 / np.sqrt(var + 1e-5), rtol=4 * U)


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_inf_in_dy_reaches_its_group_and_channel_and_nothing_else(ctx, name):
    """One inf in dy at (sample 1, channel 13), G = 8 (group 3 = channels 12..15).  Every dx element of that
    (sample, group) is non-finite (m1, m2 are); dgamma / dbeta of channels 12..15 hold non-finite values -- at
    channel 13, the only channel whose sums contain the element: a parameter gradient is a per-channel sum, so 12,
    14 and 15 keep the clean run's bits, which is asserted too.  Everything else: the clean run's bits."""
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    shape, groups = (2, 3, 5, 7, 32), 8
    x, dy, gamma, beta, _ = half_gn_case(name, shape, groups, 0.01, 21)
    assert cases.kink_free(x, groups, gamma, beta)
    bad = dy.copy()
    bad[1, 2, 3, 4, 13] = np.inf
    x_t, g_dev, b_dev = to_dev(x, dtype), f32_dev(gamma), f32_dev(beta)
    y_t, stats = gn_forward(ctx, x_t, groups, g_dev, b_dev, 0.01, code)
    out = []
    for d in (dy, bad):
        dx = torch.full_like(x_t, np.nan)
        dg, db = gn_backward(ctx, x_t, y_t, to_dev(d, dtype), dx, groups, g_dev, stats, 0.01, code)
        out.append((widen(dx), dg.cpu().numpy(), db.cpu().numpy()))
    (dx0, dg0, db0), (dx1, dg1, db1) = out
    assert np.isfinite(dx0).all() and np.isfinite(dg0).all() and np.isfinite(db0).all()
    hit = np.zeros(shape, dtype=bool)
    hit[1, ..., 12:16] = True
    assert not np.isfinite(dx1[hit]).any()
    assert np.array_equal(dx1[~hit].view(np.int32), dx0[~hit].view(np.int32))
    for g1, g0 in ((dg1, dg0), (db1, db0)):
        assert not np.isfinite(g1[12:16]).all() and not np.isfinite(g1[13])
        rest = np.arange(32) != 13
        assert np.array_equal(g1[rest].view(np.int32), g0[rest].view(np.int32))


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_backward_writes_only_its_view(ctx, name):
    """dx is a view at an 8-byte (not 16-byte) offset inside a sentinel-filled buffer."""
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    shape, groups, slope = (2, 8, 8, 8, 32), 8, 0.01
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    x, dy, gamma, beta, _ = half_gn_case(name, shape, groups, slope, 24)
    assert cases.kink_free(x, groups, gamma, beta)
    x_t, dy_t, g_dev = to_dev(x, dtype), to_dev(dy, dtype), f32_dev(gamma)
    y_t, stats = gn_forward(ctx, x_t, groups, g_dev, f32_dev(beta), slope, code)
    keep = [t.clone() for t in (x_t, y_t, dy_t, g_dev, stats)]
    plain = torch.full_like(x_t, np.nan)
    gn_backward(ctx, x_t, y_t, dy_t, plain, groups, g_dev, stats, slope, code)
    buf = torch.full((pre + n + post,), SENTINEL, dtype=dtype, device="cuda")
    view = buf[pre:pre + n].view(shape).permute(0, 4, 1, 2, 3)
    assert view.data_ptr() % 16 == 8
    gn_backward(ctx, x_t, y_t, dy_t, view, groups, g_dev, stats, slope, code)
    host = buf.float().cpu().numpy()
    assert np.all(host[:pre] == SENTINEL) and np.all(host[pre + n:] == SENTINEL)
    assert np.array_equal(host[pre:pre + n].reshape(shape).view(np.int32), widen(plain).view(np.int32))
    for t, k in zip((x_t, y_t, dy_t, g_dev, stats), keep):
        assert torch.equal(bits(t), bits(k))                # the inputs are read only


# ---- MaxPool3d(2) backward ---------------------------------------------------------------------------------
def torch_pool_backward(x, dy):
    xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 1))).requires_grad_(True)
    F.max_pool3d(xt, 2).backward(torch.from_numpy(np.ascontiguousarray(np.moveaxis(dy, -1, 1))))
    return np.moveaxis(xt.grad.numpy(), 1, -1)


def pool_check(ctx, name, x, seed):
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    x = round_to(x, dtype)
    b, d, h, w, c = x.shape
    dy = round_to(np.random.default_rng(seed).standard_normal((b, d // 2, h // 2, w // 2, c)), dtype)
    dy[dy == 0] = 1.0
    dx = torch.full((b, c, d, h, w), SENTINEL, dtype=dtype, device="cuda").contiguous(
        memory_format=torch.channels_last_3d)
    ctx.maxpool2_bwd_ndhwc(stream(), to_dev(x, dtype), to_dev(dy, dtype), dx, b, d, h, w, c, dtype=code)
    got = widen(dx)
    assert np.array_equal(got, torch_pool_backward(x, dy))
    assert np.array_equal(got, ref.maxpool2_backward(x, dy))
    for axis, n in ((1, d), (2, h), (3, w)):
        if n % 2:
            assert np.all(np.take(got, n - 1, axis=axis) == 0)
    assert np.count_nonzero(got) == dy.size


@gpu
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", cases.POOL_SHAPES)
def test_maxpool_backward(ctx, name, shape):
    pool_check(ctx, name, np.random.default_rng(31).standard_normal(shape).astype(np.float32), 32)


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_maxpool_backward_ties_and_signed_zeros(ctx, name):
    pool_check(ctx, name, cases.pool_tie_input((2, 5, 6, 7, 8), 33), 34)


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_maxpool_backward_nans(ctx, name):
    pool_check(ctx, name, cases.pool_nan_input(35), 36)


# ---- trilinear x2 up-sampling backward --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", cases.UP_SHAPES)
def test_upsample_backward(ctx, name, shape):
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    b, d, h, w, c = shape
    dy = round_to(np.random.default_rng(41).standard_normal((b, 2 * d, 2 * h, 2 * w, c)), dtype)
    want, s = ref.upsample2_trilinear_backward(dy)
    dy_t = to_dev(dy, dtype)
    dx_t = torch.full((b, c, d, h, w), np.nan, dtype=dtype, device="cuda").contiguous(
        memory_format=torch.channels_last_3d)
    ctx.upsample2_trilinear_bwd_ndhwc(stream(), dy_t, dx_t, b, d, h, w, c, dtype=code)
    dy32 = dy_t.float()
    dx32 = torch.full((b, c, d, h, w), np.nan, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    ctx.upsample2_trilinear_bwd_ndhwc(stream(), dy32, dx32, b, d, h, w, c)
    assert torch.equal(bits(dx_t), bits(dx32.to(dtype)))
    got = widen(dx_t)
    assert np.isfinite(got).all()
    bound, m32 = bound_b(want, s, widen(dx32), dtype)
    over = float((np.abs(got.astype(np.float64) - want) / bound).max())
    print(f"up {name} {shape}: m32 {m32 / U:.3f} u, half kernel {over:.3f} x bound")
    assert over <= 1.0


# ---- error codes -------------------------------------------------------------------------------------------
@gpu
def test_error_codes(ctx):
    lib = _native.lib()
    p = lambda t: int(t.data_ptr())  # noqa: E731
    x = torch.zeros(1, 32, 2, 2, 2, dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    y, big = torch.empty_like(x), torch.zeros(1, 32, 4, 4, 4, dtype=torch.float16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    stats = torch.zeros((1, 8, 2), device="cuda")
    h, s, f16 = ctx.handle, stream(), _native.DTYPE_F16

    def train(dtype, channels, groups, slope):
        return lib.exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev(h, s, dtype, p(x), p(y), 1, 8, channels, groups, None, None,
                                                              1e-5, slope, p(ws), ws.numel(), p(stats))

    def bwd(dtype, channels, groups, slope):
        return lib.exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev(h, s, dtype, p(x), p(y), p(x), p(y), 1, 8, channels, groups,
                                                            None, p(stats), slope, None, None, p(ws), ws.numel())

    for fn in (train, bwd):
        assert fn(7, 32, 8, 0.01) == -1
        assert fn(f16, 6, 1, 0.01) == -2
        assert fn(f16, 32, 8, 0.0) == -2
    assert lib.exabm4d_maxpool2_bwd_ndhwc_dt_dev(h, s, 7, p(big), p(x), p(big), 1, 4, 4, 4, 32) == -1
    assert lib.exabm4d_maxpool2_bwd_ndhwc_dt_dev(h, s, f16, p(big), p(x), p(big), 1, 4, 4, 4, 6) == -2
    assert lib.exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(h, s, 7, p(big), p(x), 1, 2, 2, 2, 32) == -1
    assert lib.exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(h, s, f16, p(big), p(x), 1, 2, 2, 2, 6) == -2
