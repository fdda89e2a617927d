"""The BM4DNet stage's NDHWC kernels (csrc/nn_kernels.hip: fused GroupNorm + conv bias + LeakyReLU,
MaxPool3d(2), trilinear x2 up-sampling) against the float64 restatement in ``nn_pyref.py``, called through the
modules ``predict`` uses (``inference.FusedGroupNormLeakyReLU``, ``inference._ResampleNDHWC``) on
``channels_last_3d`` tensors -- at the U-Net's own layer shapes, at the launch heuristics' extremes, on inputs
whose mean is large next to their spread, and on non-finite data.

The U-Net's layers at a 64^3 patch (read from ``unet3d.UNet`` and checked in ``test_layer_table``):

    GroupNorm(8, C)   32 @ 64^3 (x4), 64 @ 32^3, 128 @ 16^3, 256 @ 8^3, 256 @ 4^3, 128 @ 8^3, 64 @ 16^3, 32 @ 32^3
    max-pool input    32 @ 64^3, 64 @ 32^3, 128 @ 16^3, 256 @ 8^3
    up-sample input   256 @ 4^3, 128 @ 8^3, 64 @ 16^3, 32 @ 32^3
"""
import numpy as np
import pytest
import torch

import nn_pyref as R
from nn_grad_cases import GN_LAYERS, POOL_LAYERS, UP_LAYERS, U, gn_inputs, gn_preact_bound
from test_inference_gpu import TF_CFG

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.machine_learning import transforms as T
from aind_exaspim_image_compression.machine_learning import unet3d

pytestmark = pytest.mark.gpu


def to_dev(a):
    """numpy [b, d, h, w, c] -> a channels_last_3d fp32 CUDA tensor of shape [b, c, d, h, w]."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.permute(0, 4, 1, 2, 3)


def to_host(t):
    """[b, c, d, h, w] tensor -> numpy [b, d, h, w, c]."""
    return t.permute(0, 2, 3, 4, 1).contiguous().cpu().numpy()


# ---- GroupNorm + LeakyReLU --------------------------------------------------------------------------------

def gn_bound(x, groups, gamma, beta, eps, slope, cbias):
    """Per-element bound on |y - y64| that the fused fp32 form can meet when its statistics are right.

    The kernels evaluate, with ``rstd``, ``mean`` from the statistics (fp64) rounded to fp32,
        a = fl(rstd * gamma),  shift = fl(beta + fl(a * fl(cbias - mean))),  z' = fma(x, a, shift),
    then the LeakyReLU.  Let a, mu, z be the fp64 quantities (``nn_pyref.group_norm_parts``) and u = 2^-24.
    An error in ``a`` enters ``x * a`` and ``a * (cbias - mean)`` alike and cancels up to a relative error
    of |z - beta|; the fma rounds once.  First order, per rounding: mean u|a mu|; cbias - mean u|a cb| + u|a mu|;
    the product u|a cb| + u|a mu|; the sum u(|beta| + |a cb| + |a mu|); the fma u|z|; a = rstd gamma (two
    roundings) 2u|z - beta| <= 2u(|z| + |beta|).  That is u (3|a mu| + 3|a cb| + 3|beta| + 3|z|).  Correct
    statistics from fp32 partial sums add a relative error of a few u to rstd (-> |z - beta|) and a mean error
    of a few u of the group's std (-> |gamma|, since a * std <= |gamma|).  Hence, on the pre-activation,
        E = u (4|a mu| + 4|a cb| + 16 (|z| + |beta| + |gamma|))
    -- which the framework's own NCDHW GroupNorm meets as well (checked on every input below).  The activation
    multiplies E by the slope where z < -E (plus the rounding of that product, u |y|) and passes it where
    |z| <= E (a sign change moves y by at most max(1, slope) E).  What the bound rejects: a relative error of
    rstd growing like (mean / std)^2 u, the cancellation of sums of squares formed around zero."""
    z, E = gn_preact_bound(x, groups, gamma, beta, eps, cbias)
    y = R.leaky_relu(z, slope)
    scale = np.where(z < -E, slope, max(1.0, slope))
    return y, scale * E + U * np.abs(y)


def run_fused(x_dev, groups, gamma, beta, slope, cbias, eps=1e-5):
    """``FusedGroupNormLeakyReLU`` in place on ``x_dev``; asserts the native path ran (the result is the input)."""
    c = int(x_dev.shape[1])
    norm = torch.nn.GroupNorm(groups, c, eps=eps, affine=gamma is not None).cuda()
    if gamma is not None:
        with torch.no_grad():
            norm.weight.copy_(torch.from_numpy(np.asarray(gamma, np.float32)))
            norm.bias.copy_(torch.from_numpy(np.asarray(beta, np.float32)))
    act = torch.nn.LeakyReLU(slope)
    cb = None if cbias is None else torch.nn.Parameter(torch.from_numpy(np.asarray(cbias, np.float32)).cuda())
    mod = inference.FusedGroupNormLeakyReLU(norm, act, cb).eval()
    with torch.no_grad():
        y = mod(x_dev)
        assert y.data_ptr() == x_dev.data_ptr(), "the fused kernels did not run"
    return y, norm, act, cb


def framework_gn(x_host, norm, act, cb):
    with torch.no_grad():
        t = to_dev(x_host).contiguous()
        if cb is not None:
            t = t + cb.view(1, -1, 1, 1, 1)
        return to_host(act(norm(t)))


def check_gn(x, groups, gamma=None, beta=None, slope=0.01, cbias=None, samples=None, framework=True, label=""):
    """Run the fused module on x (numpy [b, ..., c] fp32), compare with the fp64 reference under gn_bound, and
    the framework's NCDHW GroupNorm under the same bound.  ``samples``: the batch entries to compare."""
    y_dev, norm, act, cb = run_fused(to_dev(x), groups, gamma, beta, slope, cbias)
    got = to_host(y_dev)
    del y_dev
    sel = slice(None) if samples is None else list(samples)
    want, bound = gn_bound(x[sel], groups, gamma, beta, 1e-5, slope, cbias)
    worst = _excess(got[sel], want, bound)
    assert worst <= 1.0, f"{label}: fused GroupNorm error {worst:.3g} x the bound"
    if framework:
        fw = framework_gn(x[sel], norm, act, cb)
        fw_worst = _excess(fw, want, bound)
        assert fw_worst <= 1.0, f"{label}: the framework's GroupNorm misses the bound ({fw_worst:.3g} x): bound wrong"
    return got


def _excess(got, want, bound):
    """max |got - want| / bound over finite reference values; NaN placement must match exactly."""
    nan_w = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan_w)
    fin = ~nan_w
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    return float(np.max(err / bound[fin])) if err.size else 0.0


def params(c, seed, neg_gamma=False):
    rng = np.random.default_rng(seed)
    gamma = (rng.standard_normal(c) * 0.5 + 1.0).astype(np.float32)
    if neg_gamma:
        gamma = -np.abs(gamma)
    beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    return gamma, beta


def test_layer_table():
    """The shapes the tests below use are the U-Net's own (a 64^3 patch through unet3d.UNet)."""
    model = unet3d.UNet().cuda().eval()
    seen = {"gn": [], "pool": [], "up": []}
    hooks = []
    for m in model.modules():
        kind = {torch.nn.GroupNorm: "gn", torch.nn.MaxPool3d: "pool", torch.nn.Upsample: "up"}.get(type(m))
        if kind:
            hooks.append(m.register_forward_hook(
                lambda mod, inp, out, kind=kind: seen[kind].append((int(inp[0].shape[1]), int(inp[0].shape[2])))))
            if kind == "gn":
                assert m.num_groups == 8
    with torch.no_grad():
        model(torch.zeros(1, 1, 64, 64, 64, device="cuda"))
    for h in hooks:
        h.remove()
    assert sorted(set(seen["gn"])) == sorted(GN_LAYERS) and seen["gn"].count((32, 64)) == 4 and len(seen["gn"]) == 18
    assert seen["pool"] == POOL_LAYERS and seen["up"] == UP_LAYERS


@pytest.mark.parametrize("kind", ["today", "mean10", "mean100", "mean1000", "std1e-2", "std1e-3", "constant",
                                  "spread"])
def test_groupnorm_statistics_at_64cubed(kind):
    """One sample of the U-Net's inc / up4 layer (32 channels at 64^3, G = 8 -- the 64-chunk statistics regime)
    for inputs whose mean is large next to their spread; with the conv bias folded in for half the cases."""
    x = gn_inputs(kind, (1, 64, 64, 64, 32), 8, len(kind) * 31 + ord(kind[-1]))
    gamma, beta = params(32, 1)
    cbias = (np.random.default_rng(2).standard_normal(32) * 2).astype(np.float32) if kind in ("mean100", "spread") else None
    got = check_gn(x, 8, gamma, beta, 0.01, cbias, label=kind)
    if kind == "constant":                       # every group constant: y = lrelu(beta) to rounding
        np.testing.assert_allclose(got[0, 5, 7, 9], np.where(beta > 0, beta, 0.01 * beta), rtol=0, atol=1e-3)


@pytest.mark.parametrize("c,n", GN_LAYERS)
def test_groupnorm_layer_table(c, n):
    """Every GroupNorm layer shape of the U-Net at batch 2: sample 0 today's input with a spread-out conv bias,
    sample 1 mean 100 with std 1 and negative gamma."""
    x = np.concatenate([gn_inputs("today", (1, n, n, n, c), 8, c), gn_inputs("mean100", (1, n, n, n, c), 8, c + 1)])
    cbias = (np.random.default_rng(c).standard_normal(c) * 20).astype(np.float32)
    gamma, beta = params(c, c, neg_gamma=(c % 64 == 0))
    check_gn(x, 8, gamma, beta, 0.01, cbias, label=f"{c}@{n}^3")


def test_groupnorm_batch32_and_run_to_run():
    """The bench's batch at the 64^3 layer: a different distribution in each of several samples; two runs give
    identical bytes (the partial sums are combined in a fixed order)."""
    kinds = ["today", "mean10", "mean100", "mean1000", "std1e-2", "std1e-3", "constant", "spread"]
    x = np.concatenate([gn_inputs(kinds[i % len(kinds)], (1, 64, 64, 64, 32), 8, 100 + i) for i in range(32)])
    gamma, beta = params(32, 3)
    cbias = (np.random.default_rng(4).standard_normal(32)).astype(np.float32)
    got = check_gn(x, 8, gamma, beta, 0.01, cbias, samples=[1, 2, 3, 4, 5, 6, 30, 31], framework=False,
                   label="batch 32")
    again, _, _, _ = run_fused(to_dev(x), 8, gamma, beta, 0.01, cbias)
    np.testing.assert_array_equal(to_host(again).view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("shape,groups", [
    ((2, 4, 4, 4, 1024), 8),      # 256 float4 lanes: one row per iteration
    ((2, 8, 8, 8, 16), 4),        # C = 16, G = 4: one float4 lane per group
    ((3, 1, 1, 1, 64), 8),        # spatial = 1
    ((2, 2, 4, 5, 32), 8),        # spatial 40 < 2 rows per iteration (32): a single chunk
    ((1, 6, 5, 7, 128), 8),       # batch 1, odd extents
    ((5, 3, 9, 4, 256), 8),
])
def test_groupnorm_launch_extremes(shape, groups):
    x = np.concatenate([gn_inputs("mean100", (1,) + shape[1:], groups, 7),
                        gn_inputs("std1e-3", (shape[0] - 1,) + shape[1:], groups, 8)])
    gamma, beta = params(shape[-1], 5)
    check_gn(x, groups, gamma, beta, 0.2, None, label=str(shape))


@pytest.mark.parametrize("affine,slope,neg", [(False, 0.01, False), (True, 0.2, True), (True, 1.0, False),
                                              (False, 1.0, False)])
def test_groupnorm_options(affine, slope, neg):
    x = gn_inputs("mean10", (2, 16, 16, 16, 64), 8, 9)
    gamma, beta = params(64, 6, neg_gamma=neg) if affine else (None, None)
    check_gn(x, 8, gamma, beta, slope, None, label=f"affine={affine} slope={slope}")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_groupnorm_non_finite_poisons_one_group(bad):
    """A NaN / +inf / -inf in one group of one sample: that group comes out NaN (as in the framework, not
    -inf); the other groups and samples are computed as without it."""
    x = gn_inputs("today", (2, 16, 16, 16, 32), 8, 10)
    x[1, 3, 4, 5, 13] = bad                                 # sample 1, group 3 (channels 12..15)
    gamma, beta = params(32, 7)
    got = check_gn(x, 8, gamma, beta, 0.01, None, label=f"non-finite {bad}")
    assert np.all(np.isnan(got[1, ..., 12:16]))
    got[1, ..., 12:16] = 0
    assert np.all(np.isfinite(got))


def test_groupnorm_writes_only_its_view():
    """In place on a view inside a larger buffer: the bytes before and after the view stay as they were."""
    shape = (2, 8, 8, 8, 32)
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    buf = torch.full((pre + n + post,), -7.25, dtype=torch.float32, device="cuda")
    x = gn_inputs("mean10", shape, 8, 11)
    view = buf[pre:pre + n].view(shape)
    view.copy_(torch.from_numpy(x))
    gamma, beta = params(32, 8)
    y, _, _, _ = run_fused(view.permute(0, 4, 1, 2, 3), 8, gamma, beta, 0.01, None)
    host = buf.cpu().numpy()
    assert np.all(host[:pre] == -7.25) and np.all(host[pre + n:] == -7.25)
    want, bound = gn_bound(x, 8, gamma, beta, 1e-5, 0.01, None)
    assert _excess(host[pre:pre + n].reshape(shape), want, bound) <= 1.0


def test_groupnorm_out_of_place():
    """y != x (the header's "y may be x"; what the shadow runs for a pair that does not sit right behind a
    convolution): into a view inside a larger buffer, y is within the bound, x is bit-unchanged and the bytes
    before and after y stay as they were; the module with ``inplace=False`` returns a new NDHWC tensor holding
    the same bytes, through the native entry, and leaves its input alone."""
    shape = (2, 8, 8, 8, 32)
    n = int(np.prod(shape))
    pre, post = 4096 + 4, 4096
    buf = torch.full((pre + n + post,), -7.25, dtype=torch.float32, device="cuda")
    y = buf[pre:pre + n].view(shape).permute(0, 4, 1, 2, 3)
    x = gn_inputs("mean10", shape, 8, 12)
    gamma, beta = params(32, 9)
    cbias = (np.random.default_rng(13).standard_normal(32) * 3).astype(np.float32)
    x_dev = to_dev(x)
    x0 = x_dev.clone()
    norm = torch.nn.GroupNorm(8, 32).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy(gamma))
        norm.bias.copy_(torch.from_numpy(beta))
    cb = torch.nn.Parameter(torch.from_numpy(cbias).cuda())
    need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(2, 512, 32, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _native.context(0).groupnorm_lrelu_ndhwc(torch.cuda.current_stream().cuda_stream, x_dev, y, 2, 512, 32, 8,
                                             norm.weight, norm.bias, 1e-5, 0.01, ws, need, cb)
    host = buf.cpu().numpy()
    assert np.all(host[:pre] == -7.25) and np.all(host[pre + n:] == -7.25)
    assert torch.equal(x_dev.view(torch.int32), x0.view(torch.int32))
    want, bound = gn_bound(x, 8, gamma, beta, 1e-5, 0.01, cbias)
    got = host[pre:pre + n].reshape(shape)
    assert _excess(got, want, bound) <= 1.0
    calls = []
    real = _native.Context.groupnorm_lrelu_ndhwc
    _native.Context.groupnorm_lrelu_ndhwc = lambda self, *a, **k: (calls.append(a[1:3]), real(self, *a, **k))[1]
    try:
        with torch.no_grad():
            out = inference.FusedGroupNormLeakyReLU(norm, torch.nn.LeakyReLU(0.01), cb, inplace=False).eval()(x_dev)
    finally:
        _native.Context.groupnorm_lrelu_ndhwc = real
    assert len(calls) == 1 and calls[0][0] is x_dev and calls[0][1] is out
    assert out.data_ptr() != x_dev.data_ptr() and out.is_contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(x_dev.view(torch.int32), x0.view(torch.int32))
    np.testing.assert_array_equal(to_host(out).view(np.int32), got.view(np.int32))


# ---- MaxPool3d(2) ------------------------------------------------------------------------------------------

def pool_module():
    m = inference._ResampleNDHWC(torch.nn.MaxPool3d(2)).eval()
    assert m.kind == "pool"
    return m


def up_module():
    m = inference._ResampleNDHWC(torch.nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True)).eval()
    assert m.kind == "up"
    return m


def pool_data(shape, seed):
    """Random data with many ties, both zeros, and a few NaN / +-inf."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-20, 21, size=shape) * 0.25).astype(np.float32)
    z = x == 0
    x[z] = np.where(rng.random(np.count_nonzero(z)) < 0.5, np.float32(-0.0), np.float32(0.0))
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(3, flat.size // 1000), replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=idx.size)
    return x


def run_pool(x):
    with torch.no_grad():
        y = pool_module()(to_dev(x))
    assert y.is_contiguous(memory_format=torch.channels_last_3d)
    return to_host(y)


def assert_same_bits(got, want):
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("c,n", POOL_LAYERS)
def test_maxpool_layer_table(c, n):
    x = pool_data((2, n, n, n, c), c)
    assert_same_bits(run_pool(x), R.maxpool2(x))


@pytest.mark.parametrize("shape", [(1, 7, 5, 9, 4), (3, 2, 3, 2, 8), (2, 4, 4, 4, 1024), (1, 65, 3, 33, 12)])
def test_maxpool_odd_extents_and_lane_counts(shape):
    x = pool_data(shape, sum(shape))
    assert_same_bits(run_pool(x), R.maxpool2(x))


def test_maxpool_nan_inf_and_signed_zero_in_every_window_position():
    """Channel 0: a NaN at window position k among finite values; 1: +inf at k; 2: -inf at k, rest -5;
    3: -0 at k, +0 elsewhere; 4..7: +0 at k, -0 elsewhere."""
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
    got = run_pool(x)
    assert_same_bits(got, R.maxpool2(x))
    assert np.all(np.isnan(got[..., 0])) and np.all(got[..., 1] == np.inf) and np.all(got[..., 2] == -5.0)
    assert_same_bits(got, to_host(torch.nn.functional.max_pool3d(to_dev(x).contiguous(), 2)))


# ---- trilinear x2 up-sampling -------------------------------------------------------------------------------

def _corner_max(v):
    """For every output of the x2 interpolation of v[b, d, h, w, c]: the max of v over the 8 corners the
    exact-ratio reference reads."""
    (d0, d1, _, _), (h0, h1, _, _), (w0, w1, _, _) = (R._up_axis(n) for n in v.shape[1:4])
    t = np.maximum(v[:, :, :, w0], v[:, :, :, w1])
    t = np.maximum(t[:, :, h0], t[:, :, h1])
    return np.maximum(t[:, d0], t[:, d1])


def up_bound(x):
    """|y - y64| for the kernel's fp32 evaluation at fp32 source coordinates.  Rounding: three levels of
    w0 a + w1 c with w0 = fl(1 - w1), at most 8u of the largest |corner| M.  Coordinate: r = (in - 1)/(out - 1)
    rounded to fp32 and src = fl(r o) are within u src <= u (in - 1) of the exact ones, and may fall into the
    neighbouring cell next to an integer; the value moves by that times the largest difference G of adjacent
    inputs along the axis over the cells either side of the corners.  Bound: u (8 M + 2 sum_axes (in - 1) G)."""
    x = np.asarray(x, np.float64)
    M = _corner_max(np.abs(x))
    E = 8 * M
    for ax in (1, 2, 3):
        n = x.shape[ax]
        if n < 2:
            continue
        g = np.abs(np.diff(x, axis=ax))
        lo = np.concatenate([np.take(g, [0], axis=ax), g], axis=ax)       # cell before index j
        hi = np.concatenate([g, np.take(g, [n - 2], axis=ax)], axis=ax)   # cell after index j
        E = E + 2 * (n - 1) * _corner_max(np.maximum(lo, hi))
    return U * E


def run_up(x_dev):
    with torch.no_grad():
        y = up_module()(x_dev)
    assert y.is_contiguous(memory_format=torch.channels_last_3d)
    return y


def check_up(x):
    x_dev = to_dev(x)
    got = to_host(run_up(x_dev))
    with torch.no_grad():
        fw = to_host(torch.nn.functional.interpolate(x_dev.contiguous(), scale_factor=2, mode="trilinear",
                                                     align_corners=True))
    # non-finite placement: the framework's (same fp32 source coordinates)
    for f in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(f(got), f(fw))
    want, bound = R.upsample2_trilinear(x), up_bound(x)
    fin = np.isfinite(want) & np.isfinite(bound) & np.isfinite(fw)
    err = np.abs(got[fin] - want[fin]) / np.maximum(bound[fin], 1e-300)
    fw_err = np.abs(fw[fin] - want[fin]) / np.maximum(bound[fin], 1e-300)
    assert err.max() <= 1.0, f"up-sampling error {err.max():.3g} x the bound"
    assert fw_err.max() <= 1.0, f"the framework misses the bound ({fw_err.max():.3g} x): bound wrong"
    return got


@pytest.mark.parametrize("c,n", UP_LAYERS)
def test_upsample_layer_table(c, n):
    x = np.random.default_rng(c).standard_normal((2, n, n, n, c), dtype=np.float32) * 3 + 1.5
    check_up(x)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 4), (2, 1, 3, 2, 4), (1, 5, 7, 3, 8), (3, 4, 4, 4, 1024),
                                   (1, 9, 2, 11, 4)])
def test_upsample_extents_and_lane_counts(shape):
    x = np.random.default_rng(sum(shape)).standard_normal(shape, dtype=np.float32) * 100
    check_up(x)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_upsample_non_finite(bad):
    x = np.random.default_rng(12).standard_normal((2, 4, 5, 6, 8), dtype=np.float32)
    x[0, 1, 2, 3, 1] = bad
    x[1, 3, 4, 5, 6] = bad                       # the far corner
    x[1, 0, 0, 0, 2] = bad
    x[1, 0, 0, 1, 2] = -bad                      # opposite infinities (NaN for bad = NaN) side by side
    got = check_up(x)
    assert np.count_nonzero(~np.isfinite(got)) > 8


# ---- index width: tensors of more than 2^31 elements -------------------------------------------------------

def _need_gib(n):
    free, _ = torch.cuda.mem_get_info()
    if free < n * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free on the device, {n} needed")


def _sample_positions(shape, count, seed):
    """``count`` random multi-indices into ``shape`` plus the last 4096 in row-major order (as int64 arrays)."""
    total = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    flat = np.concatenate([rng.integers(0, total, size=count), np.arange(total - 4096, total)])
    return np.unravel_index(flat, shape)


def test_maxpool_beyond_int32_indexing():
    """Max-pool input of 33 x 128^3 x 32 = 2.2e9 floats (8.9 GB): 10^5 random outputs and the last ones."""
    _need_gib(16)
    shape = (33, 128, 128, 128, 32)
    g = torch.Generator(device="cuda").manual_seed(13)
    xs = torch.randn(shape, generator=g, device="cuda")
    assert xs.numel() > 2 ** 31
    with torch.no_grad():
        y = pool_module()(xs.permute(0, 4, 1, 2, 3))
    ys = y.permute(0, 2, 3, 4, 1)                                       # [b, od, oh, ow, c] view
    b, od, oh, ow, c = (torch.from_numpy(i).cuda() for i in _sample_positions(tuple(ys.shape), 100_000, 14))
    win = torch.stack([xs[b, 2 * od + (k >> 2), 2 * oh + ((k >> 1) & 1), 2 * ow + (k & 1), c] for k in range(8)],
                      dim=1).cpu().numpy()                               # [n, 8] in window order
    want = R.maxpool2(win.reshape(-1, 2, 2, 2, 1)).reshape(-1)
    got = ys[b, od, oh, ow, c].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    del xs, y, ys
    torch.cuda.empty_cache()


def test_upsample_beyond_int32_indexing():
    """Up-sampling (32, 32, 64^3) -> 2^31 output floats (8 GiB): 10^5 random outputs and the last ones against the
    fp64 interpolation of their 8 corners, under ``up_bound`` with the adjacent differences bounded by twice the
    largest |x| of the tensor (addressing, not rounding, is what this checks)."""
    _need_gib(16)
    shape = (32, 64, 64, 64, 32)
    g = torch.Generator(device="cuda").manual_seed(15)
    xs = torch.randn(shape, generator=g, device="cuda")
    with torch.no_grad():
        y = up_module()(xs.permute(0, 4, 1, 2, 3))
    assert y.numel() == 2 ** 31
    ys = y.permute(0, 2, 3, 4, 1)
    pos = _sample_positions(tuple(ys.shape), 100_000, 16)
    b, od, oh, ow, c = pos
    axis = R._up_axis(64)
    (d0, d1, dw0, dw1), (h0, h1, hw0, hw1), (w0, w1, ww0, ww1) = [tuple(v[o] for v in axis) for o in (od, oh, ow)]
    dev = lambda a: torch.from_numpy(np.asarray(a)).cuda()             # noqa: E731
    corners = {}

    def at(d, h, w):
        v = xs[dev(b), dev(d), dev(h), dev(w), dev(c)].cpu().numpy().astype(np.float64)
        corners[(id(d), id(h), id(w))] = np.abs(v)
        return v
    lw = lambda d, h: ww0 * at(d, h, w0) + ww1 * at(d, h, w1)          # noqa: E731
    lh = lambda d: hw0 * lw(d, h0) + hw1 * lw(d, h1)                   # noqa: E731
    want = dw0 * lh(d0) + dw1 * lh(d1)
    got = ys[dev(b), dev(od), dev(oh), dev(ow), dev(c)].cpu().numpy()
    M = np.max(np.stack(list(corners.values())), axis=0)
    bound = U * (8 * M + 2 * 3 * 63 * 2 * float(xs.abs().max()))
    assert np.all(np.abs(got - want) <= bound)
    del xs, y, ys
    torch.cuda.empty_cache()


# ---- end to end: the NDHWC shadow of a U-Net against its fp64 forward ---------------------------------------

@pytest.mark.parametrize("inp", ["randn", "flat"])
def test_shadow_forward_against_fp64(inp):
    """A seeded random-init U-Net at 32^3, batch 1, through the fused NDHWC shadow (what ``predict`` runs)
    against ``model.double()`` on the CPU: its largest error is at most twice that of the unfused fp32 shadow
    (the framework's GroupNorm), plus a floor of 1e-5 of the output's range.  ``flat``: the training transform
    of a near-constant raw volume (background counts with +-1 noise), where the norm layers see groups with a
    large mean next to a small spread."""
    torch.manual_seed(0)
    model = unet3d.UNet().eval()
    with torch.no_grad():                                 # GroupNorm's default affine is (1, 0): make it matter
        for m in model.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
    rng = np.random.default_rng(17)
    if inp == "randn":
        x = rng.standard_normal((1, 1, 32, 32, 32)).astype(np.float32)
    else:
        raw = 110 + rng.integers(-1, 2, size=(1, 1, 32, 32, 32))
        x = np.asarray(T.build_transform(TF_CFG).forward(raw.astype(np.float32)), np.float32)
    with torch.no_grad():
        want = model.double()(torch.from_numpy(x).double()).numpy()
        model.float().cuda()
        xd = torch.from_numpy(x).cuda()
        fused = inference._ndhwc_shadow(model)(xd).cpu().numpy()
        plain = inference._ndhwc_shadow(model, fuse=False)(xd).cpu().numpy()
    assert sum(isinstance(m, inference.FusedGroupNormLeakyReLU) for m in inference._ndhwc_shadow(model).modules()) == 18
    e_fused = np.max(np.abs(fused - want))
    e_plain = np.max(np.abs(plain - want))
    floor = 1e-5 * float(np.ptp(want))
    assert e_fused <= 2 * e_plain + floor, f"fused shadow {e_fused:.3g} vs unfused {e_plain:.3g} (floor {floor:.3g})"
