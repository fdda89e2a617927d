"""BM4DNet in fp16 / bf16: the half-width NDHWC kernels (csrc/nn_kernels.hip through the ``*_dt_dev`` entries)
against the float64 restatement in ``nn_pyref.py`` of the same half-width input, and ``predict(precision=...)``
end to end against the fp32 path.

Kernel bounds.  The kernels widen the input to fp32 exactly, compute as the fp32 kernels do and round each
output once to the storage type.  So a result is within one ulp of the storage type at the reference value,
plus the fp32 evaluation's own bound (``gn_bound`` / ``up_bound`` of ``test_nn_kernels_gpu``), which only
matters next to zero, where the storage type's ulp is finer than the fp32 roundings of terms like |a * mean|.
The max-pool selects: it is bit-exact.
"""
import numpy as np
import pytest
import torch

import nn_pyref as R
from test_inference_gpu import TF_CFG
from test_nn_kernels_gpu import GN_LAYERS, POOL_LAYERS, UP_LAYERS, gn_bound, gn_inputs, params, pool_data, up_bound
from test_oracle_golden import tiling_volume

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.machine_learning import transforms as T
from aind_exaspim_image_compression.machine_learning import unet3d

pytestmark = pytest.mark.gpu
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
# (mantissa bits, smallest normal exponent) of the storage types
FORMAT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}


def ulp(v, dtype):
    """Spacing of ``dtype`` at |v| (the subnormal spacing below the smallest normal), in fp64."""
    p, emin = FORMAT[dtype]
    a = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.exp2(e - p)


def to_dev(a, dtype):
    """numpy [b, d, h, w, c] -> a channels_last_3d CUDA tensor of ``dtype``, shape [b, c, d, h, w] (rounded to
    nearest even by torch on the host)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).cuda()
    return t.permute(0, 4, 1, 2, 3)


def widen(t):
    """[b, c, d, h, w] half tensor -> numpy fp32 [b, d, h, w, c] (exact)."""
    return t.permute(0, 2, 3, 4, 1).float().contiguous().cpu().numpy()


def excess(got, want, bound):
    """max |got - want| / bound over finite reference values; NaN placement must match exactly."""
    nan_w = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan_w)
    fin = ~nan_w
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    return float(np.max(err / bound[fin])) if err.size else 0.0


# ---- GroupNorm + LeakyReLU ---------------------------------------------------------------------------------

def run_fused(x_dev, groups, gamma, beta, slope, cbias, eps=1e-5):
    """A half-enabled ``FusedGroupNormLeakyReLU`` in place on ``x_dev``; asserts the native path ran."""
    c = int(x_dev.shape[1])
    norm = torch.nn.GroupNorm(groups, c, eps=eps, affine=gamma is not None).cuda()
    if gamma is not None:
        with torch.no_grad():
            norm.weight.copy_(torch.from_numpy(np.asarray(gamma, np.float32)))
            norm.bias.copy_(torch.from_numpy(np.asarray(beta, np.float32)))
    cb = None if cbias is None else torch.nn.Parameter(torch.from_numpy(np.asarray(cbias, np.float32)).cuda())
    mod = inference.FusedGroupNormLeakyReLU(norm, torch.nn.LeakyReLU(slope), cb, half=True).eval()
    with torch.no_grad():
        y = mod(x_dev)
    assert y.data_ptr() == x_dev.data_ptr() and y.dtype == x_dev.dtype, "the fused kernels did not run"
    return y


def check_gn(x, dtype, groups, gamma=None, beta=None, slope=0.01, cbias=None, samples=None, label=""):
    """x: fp32 numpy [b, ..., c]; rounded to ``dtype``, normalised on the device, compared with the fp64 result
    of the rounded input."""
    x_dev = to_dev(x, dtype)
    xh = widen(x_dev)                                     # the half-width input, exactly
    got = widen(run_fused(x_dev, groups, gamma, beta, slope, cbias))
    sel = slice(None) if samples is None else list(samples)
    want, e32 = gn_bound(xh[sel], groups, gamma, beta, 1e-5, slope, cbias)
    worst = excess(got[sel], want, ulp(want, dtype) + e32)
    assert worst <= 1.0, f"{label}: half GroupNorm error {worst:.3g} x (1 ulp + the fp32 bound)"
    return got, xh


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("kind", ["today", "mean100", "mean1000", "std1e-2", "std1e-3", "constant", "spread"])
def test_groupnorm_statistics_at_64cubed(name, kind):
    """The 32-channel 64^3 layer, batch 1, inputs whose mean is large next to their spread; conv bias folded in
    for half the cases."""
    x = gn_inputs(kind, (1, 64, 64, 64, 32), 8, len(kind) * 31 + ord(kind[-1]))
    gamma, beta = params(32, 1)
    cbias = (np.random.default_rng(2).standard_normal(32) * 2).astype(np.float32) if kind in ("mean100", "spread") else None
    got, _ = check_gn(x, DTYPES[name], 8, gamma, beta, 0.01, cbias, label=f"{name} {kind}")
    if kind == "constant":
        np.testing.assert_allclose(got[0, 5, 7, 9], np.where(beta > 0, beta, 0.01 * beta), rtol=0, atol=1e-2)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("c,n", GN_LAYERS + [(512, 4)])
def test_groupnorm_layer_table(name, c, n):
    """Every GroupNorm layer shape of the U-Net (and C = 512) at batch 2: sample 0 today's input with a
    spread-out conv bias, sample 1 mean 100, std 1, negative gamma for half the widths."""
    x = np.concatenate([gn_inputs("today", (1, n, n, n, c), 8, c), gn_inputs("mean100", (1, n, n, n, c), 8, c + 1)])
    cbias = (np.random.default_rng(c).standard_normal(c) * 20).astype(np.float32)
    gamma, beta = params(c, c, neg_gamma=(c % 64 == 0))
    check_gn(x, DTYPES[name], 8, gamma, beta, 0.01, cbias, label=f"{name} {c}@{n}^3")


@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_batch32_and_run_to_run(name):
    """The bench's batch of 32 at the 64^3 layer, a different distribution per sample; two launches give
    identical bytes."""
    dtype = DTYPES[name]
    kinds = ["today", "mean10", "mean100", "mean1000", "std1e-2", "std1e-3", "constant", "spread"]
    x = np.concatenate([gn_inputs(kinds[i % len(kinds)], (1, 64, 64, 64, 32), 8, 100 + i) for i in range(32)])
    gamma, beta = params(32, 3)
    cbias = (np.random.default_rng(4).standard_normal(32)).astype(np.float32)
    got, _ = check_gn(x, dtype, 8, gamma, beta, 0.01, cbias, samples=[1, 2, 3, 6, 30, 31], label=f"{name} batch 32")
    again = widen(run_fused(to_dev(x, dtype), 8, gamma, beta, 0.01, cbias))
    np.testing.assert_array_equal(again.view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape,groups", [
    ((2, 4, 4, 4, 1024), 8),      # 256 lanes: one row per iteration
    ((2, 8, 8, 8, 16), 4),        # C = 16, G = 4: one lane per group
    ((3, 1, 1, 1, 64), 8),        # spatial = 1
    ((1, 6, 5, 7, 128), 8),       # batch 1, odd extents
    ((2, 33, 17, 9, 32), 8),      # odd extents at the narrowest layer's width
])
def test_groupnorm_launch_extremes_and_odd_extents(name, shape, groups):
    x = np.concatenate([gn_inputs("mean100", (1,) + shape[1:], groups, 7),
                        gn_inputs("std1e-2", (shape[0] - 1,) + shape[1:], groups, 8)])
    gamma, beta = params(shape[-1], 5)
    check_gn(x, DTYPES[name], groups, gamma, beta, 0.2, None, label=f"{name} {shape}")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("affine,cbias", [(False, False), (False, True), (True, False)])
def test_groupnorm_without_affine_or_bias(name, affine, cbias):
    x = gn_inputs("mean10", (2, 16, 16, 16, 64), 8, 9)
    gamma, beta = params(64, 6) if affine else (None, None)
    cb = (np.random.default_rng(5).standard_normal(64) * 3).astype(np.float32) if cbias else None
    check_gn(x, DTYPES[name], 8, gamma, beta, 0.01, cb, label=f"{name} affine={affine} bias={cbias}")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_groupnorm_non_finite_poisons_one_group(name, bad):
    x = gn_inputs("today", (2, 16, 16, 16, 32), 8, 10)
    x[1, 3, 4, 5, 13] = bad                               # sample 1, group 3 (channels 12..15)
    gamma, beta = params(32, 7)
    got, _ = check_gn(x, DTYPES[name], 8, gamma, beta, 0.01, None, label=f"{name} non-finite {bad}")
    assert np.all(np.isnan(got[1, ..., 12:16]))
    got[1, ..., 12:16] = 0
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_writes_only_its_view(name):
    """In place on a view inside a larger buffer (at an 8-byte, not 16-byte, offset): the elements before and
    after the view stay as they were."""
    dtype = DTYPES[name]
    shape = (2, 8, 8, 8, 32)
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    buf = torch.full((pre + n + post,), -7.25, dtype=dtype, device="cuda")
    x = gn_inputs("mean10", shape, 8, 11)
    view = buf[pre:pre + n].view(shape)
    view.copy_(torch.from_numpy(x).to(dtype))
    xh = view.float().cpu().numpy()
    gamma, beta = params(32, 8)
    run_fused(view.permute(0, 4, 1, 2, 3), 8, gamma, beta, 0.01, None)
    host = buf.float().cpu().numpy()
    assert np.all(host[:pre] == -7.25) and np.all(host[pre + n:] == -7.25)
    want, e32 = gn_bound(xh, 8, gamma, beta, 1e-5, 0.01, None)
    assert excess(host[pre:pre + n].reshape(shape), want, ulp(want, dtype) + e32) <= 1.0


@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_out_of_place(name):
    """y != x in the half types: into a view at an 8-byte offset inside a larger buffer, y is within 1 ulp + the
    fp32 bound, x is bit-unchanged and the elements before and after y stay as they were; the module with
    ``inplace=False`` returns a new NDHWC tensor holding the same bits, through the native entry."""
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    shape = (2, 8, 8, 8, 32)
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    buf = torch.full((pre + n + post,), -7.25, dtype=dtype, device="cuda")
    y = buf[pre:pre + n].view(shape).permute(0, 4, 1, 2, 3)
    x_dev = to_dev(gn_inputs("mean10", shape, 8, 12), dtype)
    xh = widen(x_dev)
    x0 = x_dev.clone()
    gamma, beta = params(32, 9)
    cbias = (np.random.default_rng(13).standard_normal(32) * 3).astype(np.float32)
    norm = torch.nn.GroupNorm(8, 32).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy(gamma))
        norm.bias.copy_(torch.from_numpy(beta))
    cb = torch.nn.Parameter(torch.from_numpy(cbias).cuda())
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(2, 512, 32, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _native.context(0).groupnorm_lrelu_ndhwc(torch.cuda.current_stream().cuda_stream, x_dev, y, 2, 512, 32, 8,
                                             norm.weight, norm.bias, 1e-5, 0.01, ws, need, cb, dtype=code)
    host = buf.float().cpu().numpy()
    assert np.all(host[:pre] == -7.25) and np.all(host[pre + n:] == -7.25)
    assert torch.equal(x_dev.view(torch.int16), x0.view(torch.int16))
    want, e32 = gn_bound(xh, 8, gamma, beta, 1e-5, 0.01, cbias)
    got = host[pre:pre + n].reshape(shape)
    assert excess(got, want, ulp(want, dtype) + e32) <= 1.0
    mod = inference.FusedGroupNormLeakyReLU(norm, torch.nn.LeakyReLU(0.01), cb, half=True, inplace=False).eval()
    with torch.no_grad():
        seen, out = _count_native(lambda: mod(x_dev))
    assert seen["gn"] == [code]
    assert out.dtype == dtype and out.data_ptr() != x_dev.data_ptr()
    assert out.is_contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(x_dev.view(torch.int16), x0.view(torch.int16))
    np.testing.assert_array_equal(widen(out).view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("name", DTYPES)
def test_unsupported_shapes_and_framework_fallback(name):
    """Channel counts the kernels do not take: the entries return EXABM4D_ERR_UNSUPPORTED, and the modules give
    the framework's result on the same half tensor."""
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    lib, ctx = _native.lib(), _native.context(0)
    x = to_dev(gn_inputs("today", (1, 4, 4, 4, 12), 3, 12), dtype)        # 12 channels: 256 % 3 != 0
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.exabm4d_groupnorm_lrelu_ndhwc_dt_dev(ctx.handle, stream, code, x.data_ptr(), x.data_ptr(), 1, 64, 12, 3,
                                                 None, None, 1e-5, 0.01, ws.data_ptr(), ws.numel(), None)
    assert rc == -2
    y6 = torch.empty(1, 6, 2, 2, 2, dtype=dtype, device="cuda")
    x6 = torch.zeros(1, 6, 4, 4, 4, dtype=dtype, device="cuda")
    assert lib.exabm4d_maxpool2_ndhwc_dt_dev(ctx.handle, stream, code, x6.data_ptr(), y6.data_ptr(), 1, 4, 4, 4, 6) == -2
    assert lib.exabm4d_upsample2_trilinear_ndhwc_dt_dev(ctx.handle, stream, code, x6.data_ptr(), y6.data_ptr(), 1,
                                                        1, 1, 1, 6) == -2
    assert lib.exabm4d_maxpool2_ndhwc_dt_dev(ctx.handle, stream, 7, x6.data_ptr(), y6.data_ptr(), 1, 4, 4, 4, 8) == -1

    norm = torch.nn.GroupNorm(3, 12).cuda().to(dtype)
    mod = inference.FusedGroupNormLeakyReLU(norm, torch.nn.LeakyReLU(0.01), half=True).eval()
    with torch.no_grad():
        want = torch.nn.functional.leaky_relu(norm(x.clone()), 0.01)
        got = mod(x.clone())
    assert got.dtype == dtype
    np.testing.assert_array_equal(got.float().cpu().numpy(), want.float().cpu().numpy())
    pool = inference._ResampleNDHWC(torch.nn.MaxPool3d(2), half=True).eval()
    xr = torch.randn(1, 6, 4, 4, 4, device="cuda").to(dtype).to(memory_format=torch.channels_last_3d)
    with torch.no_grad():
        np.testing.assert_array_equal(pool(xr).float().cpu().numpy(),
                                      torch.nn.functional.max_pool3d(xr.contiguous(), 2).float().cpu().numpy())


# ---- MaxPool3d(2) ------------------------------------------------------------------------------------------

def run_pool(x_dev):
    m = inference._ResampleNDHWC(torch.nn.MaxPool3d(2), half=True).eval()
    with torch.no_grad():
        y = m(x_dev)
    assert y.dtype == x_dev.dtype and y.is_contiguous(memory_format=torch.channels_last_3d)
    return y


def assert_pool_exact(x_dev):
    got = run_pool(x_dev)
    fw = torch.nn.functional.max_pool3d(x_dev.contiguous(), 2)
    g, f = widen(got), widen(fw)
    want = R.maxpool2(widen(x_dev))                       # selects: exact on the widened values
    for other in (f, want):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(other))
        fin = ~np.isnan(g)
        np.testing.assert_array_equal(g[fin].view(np.int32), other[fin].view(np.int32))   # incl. the sign of 0
    return g


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("c,n", POOL_LAYERS)
def test_maxpool_layer_table(name, c, n):
    assert_pool_exact(to_dev(pool_data((2, n, n, n, c), c), DTYPES[name]))


@pytest.mark.parametrize("name", DTYPES)
def test_maxpool_batch32(name):
    assert_pool_exact(to_dev(pool_data((32, 64, 64, 64, 32), 32), DTYPES[name]))


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", [(1, 7, 5, 9, 4), (3, 2, 3, 2, 8), (2, 4, 4, 4, 1024), (1, 65, 3, 33, 12)])
def test_maxpool_odd_extents_and_lane_counts(name, shape):
    assert_pool_exact(to_dev(pool_data(shape, sum(shape)), DTYPES[name]))


@pytest.mark.parametrize("name", DTYPES)
def test_maxpool_nan_inf_and_signed_zero_in_every_window_position(name):
    x = np.full((8, 2, 2, 2, 8), 1.0, np.float32)
    x[..., 2] = -5.0
    x[..., 3] = 0.0
    x[..., 4:] = -0.0
    for k in range(8):
        p = (k, k >> 2, (k >> 1) & 1, k & 1)
        x[p + (0,)] = np.nan
        x[p + (1,)] = np.inf
        x[p + (2,)] = -np.inf
        x[p + (3,)] = -0.0
        x[p + (slice(4, 8),)] = 0.0
    got = assert_pool_exact(to_dev(x, DTYPES[name]))
    assert np.all(np.isnan(got[..., 0])) and np.all(got[..., 1] == np.inf) and np.all(got[..., 2] == -5.0)
    assert np.all(np.signbit(got[..., 3]) == (np.arange(8) == 0)[:, None, None, None])


# ---- trilinear x2 up-sampling -------------------------------------------------------------------------------

def check_up(x, dtype):
    x_dev = to_dev(x, dtype)
    xh = widen(x_dev)
    m = inference._ResampleNDHWC(torch.nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
                                 half=True).eval()
    with torch.no_grad():
        y = m(x_dev)
        fw = widen(torch.nn.functional.interpolate(x_dev.contiguous(), scale_factor=2, mode="trilinear",
                                                   align_corners=True))
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last_3d)
    got = widen(y)
    for f in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(f(got), f(fw))
    want = R.upsample2_trilinear(xh)
    bound = ulp(want, dtype) + up_bound(xh)
    fin = np.isfinite(want) & np.isfinite(bound) & np.isfinite(fw)
    err = np.abs(got[fin] - want[fin]) / bound[fin]
    assert err.max() <= 1.0, f"half up-sampling error {err.max():.3g} x (1 ulp + the fp32 bound)"
    return got


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("c,n", UP_LAYERS)
def test_upsample_layer_table(name, c, n):
    x = np.random.default_rng(c).standard_normal((2, n, n, n, c), dtype=np.float32) * 3 + 1.5
    check_up(x, DTYPES[name])


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 4), (2, 1, 3, 2, 4), (1, 5, 7, 3, 8), (3, 4, 4, 4, 1024),
                                   (1, 9, 2, 11, 4)])
def test_upsample_extents_and_lane_counts(name, shape):
    x = np.random.default_rng(sum(shape)).standard_normal(shape, dtype=np.float32) * 100
    check_up(x, DTYPES[name])


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_upsample_non_finite(name, bad):
    x = np.random.default_rng(12).standard_normal((2, 4, 5, 6, 8), dtype=np.float32)
    x[0, 1, 2, 3, 1] = bad
    x[1, 3, 4, 5, 6] = bad
    got = check_up(x, DTYPES[name])
    assert np.count_nonzero(~np.isfinite(got)) > 8


# ---- end to end ---------------------------------------------------------------------------------------------

def _count_native(fn):
    """Run fn() and return the dtype codes the three native NDHWC entries were called with, per entry."""
    seen = {"gn": [], "pool": [], "up": []}
    C = _native.Context
    real = {"gn": C.groupnorm_lrelu_ndhwc, "pool": C.maxpool2_ndhwc, "up": C.upsample2_trilinear_ndhwc}

    def spy(kind):
        def f(self, *a, **k):
            seen[kind].append(k.get("dtype"))
            return real[kind](self, *a, **k)
        return f
    C.groupnorm_lrelu_ndhwc, C.maxpool2_ndhwc, C.upsample2_trilinear_ndhwc = spy("gn"), spy("pool"), spy("up")
    try:
        out = fn()
    finally:
        C.groupnorm_lrelu_ndhwc, C.maxpool2_ndhwc, C.upsample2_trilinear_ndhwc = real["gn"], real["pool"], real["up"]
    return seen, out


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("net,fused,pools", [("UNet", 18, 4), ("N2V2UNet", 17, 0)])
def test_predict_runs_every_layer_native_in_half(name, net, fused, pools):
    """predict(precision=p) on one 64^3 patch: the GroupNorm pairs fused and every max-pool / up-sampling native,
    in p; for the U-Net all 18 pairs, and every convolution after the first sees a half-width NDHWC input (no
    NCDHW copies).  N2V2: its MaxBlurPool stays on the framework, and so does the one norm layer the kernels do
    not take, GroupNorm(8, 16) in front of the last up-sampling block's second convolution (two channels per
    group), as in fp32."""
    dtype = DTYPES[name]
    torch.manual_seed(0)
    model = getattr(unet3d, net)().cuda().eval()
    convs = []
    orig_conv = torch.nn.Conv3d.forward

    def conv_spy(self, x):
        convs.append((x.dtype, x.shape[1] == 1 or x.is_contiguous(memory_format=torch.channels_last_3d)))
        return orig_conv(self, x)
    torch.nn.Conv3d.forward = conv_spy
    try:
        seen, out = _count_native(lambda: inference.predict(tiling_volume((64, 64, 64), seed=5), model,
                                                            T.build_transform(TF_CFG), verbose=False,
                                                            precision=name))
    finally:
        torch.nn.Conv3d.forward = orig_conv
    code = inference._NATIVE_DTYPES[dtype]
    assert seen["gn"] == [code] * fused
    assert seen["pool"] == [code] * pools and seen["up"] == [code] * 4
    # the first convolution takes the fp32 batch (one channel: NCDHW and NDHWC alike) and casts it itself
    assert len(convs) == 19 and convs[0] == (torch.float32, True), convs
    if net == "UNet":
        assert all(c == (dtype, True) for c in convs[1:]), convs
    assert out.shape == (64, 64, 64) and out.dtype == np.uint16


def test_callers_own_autocast_keeps_todays_path():
    """A caller's autocast around today's fp32 shadow: no half-width tensor reaches the native entries (the norm
    pairs fall back to the framework exactly as before this feature; what reaches the entries is fp32)."""
    torch.manual_seed(0)
    shadow = inference._ndhwc_shadow(unet3d.UNet().cuda().eval())
    x = torch.randn(1, 1, 16, 16, 16, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        seen, _ = _count_native(lambda: shadow(x))
    assert not seen["gn"] and set(seen["pool"] + seen["up"]) <= {_native.DTYPE_F32}


CEILING = {"fp16": 1e-2, "bf16": 5e-2}


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("net", ["UNet", "N2V2UNet"])
def test_half_correction_against_fp32(name, net):
    """The network's correction (output - input) on a 64^3 patch, half shadow against the fp32 shadow, for the
    seeded (golden) states: max |delta| <= ceiling x max |correction|.  The output stays fp32 (the residual sum)."""
    torch.manual_seed(0)
    model = getattr(unet3d, net)().cuda().eval()
    x = torch.randn(2, 1, 64, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        ref = inference._ndhwc_shadow(model)(x)
        with torch.autocast("cuda", dtype=DTYPES[name]):
            half = inference._ndhwc_shadow(model, half=True)(x)
    assert half.dtype == torch.float32 and ref.dtype == torch.float32
    corr = (ref - x).double()
    delta = float(((half - x).double() - corr).abs().max())
    ratio = delta / float(corr.abs().max())
    print(f"{net} {name}: max |delta correction| = {delta:.4g} = {ratio:.3g} x max |correction|")
    assert np.isfinite(ratio) and ratio <= CEILING[name], f"{net} {name}: {ratio:.3g} > {CEILING[name]}"


@pytest.fixture(scope="module")
def vol128():
    torch.manual_seed(0)
    model = unet3d.UNet().cuda().eval()
    vol = tiling_volume((128, 128, 128), seed=6)
    tf = T.build_transform(TF_CFG)
    return model, vol, tf, inference.predict(vol, model, tf, verbose=False)


@pytest.mark.parametrize("name", DTYPES)
def test_predict_128_in_half(vol128, name):
    model, vol, tf, ref = vol128
    out = inference.predict(vol, model, tf, verbose=False, precision=name)
    assert out.shape == vol.shape and out.dtype == np.uint16
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    print(f"predict 128^3 {name} vs fp32: mean |delta counts| {d.mean():.4g}, max {d.max()}, "
          f"fp32 range {ref.min()}..{ref.max()}")
    assert np.all(out[:5] == ref[:5])                     # the zero-weight margin: transform.inverse(0) either way


def test_predict_fp32_is_todays_predict(vol128):
    model, vol, tf, ref = vol128
    np.testing.assert_array_equal(inference.predict(vol, model, tf, verbose=False, precision="fp32"), ref)


@pytest.mark.parametrize("name", DTYPES)
def test_predict_half_with_a_callable_and_fast_off(name):
    """fast=False / a plain callable: autocast around each call; the result is still uint16 of the right shape
    and close to fp32."""
    torch.manual_seed(0)
    model = unet3d.UNet().cuda().eval()
    tf = T.build_transform(TF_CFG)
    vol = tiling_volume((64, 64, 64), seed=7)
    ref = inference.predict(vol, model, tf, verbose=False, fast=False).astype(np.int64)
    for m in (model, lambda b: model(b)):
        out = inference.predict(vol, m, tf, verbose=False, fast=False, precision=name)
        assert out.shape == vol.shape and out.dtype == np.uint16
        assert np.mean(np.abs(out.astype(np.int64) - ref)) < 0.05 * np.mean(np.abs(ref - 37))
