"""The training backward kernels (csrc/nn_grad_kernels.hip) where a wrong gradient would go unnoticed: on the
input distributions that amplify an error of the statistics, at the U-Net's own layer shapes, past the launch caps,
on dead channels, on non-finite data, and through the autograd wrappers of ``inference.py``.  The helpers are those
of ``test_nn_grad_gpu`` (fp32) and ``test_nn_grad_half_gpu`` (fp16 / bf16).

Every GroupNorm case asserts three things, in this order (u = 2^-24; S = the reference on the absolute values of
its summands, ``nn_grad_pyref``; ``measure`` = max |got - ref| / S, exactly 0 demanded where S == 0).

(a) The statistics the backward consumes.  ``stats`` of the training forward against fp64 at the tolerances of
    ``test_forward_statistics_are_the_forwards_own``: |mean - mean64| <= 4u max|x| (max over the sample),
    |rstd - rstd64| <= 4u rstd64.

(b) Given those statistics, the backward is right to rounding: against the CONDITIONAL reference -- the fp64
    formulas fed with the fp32 (mean, rstd) read back from the device -- measure(dx), measure(dgamma),
    measure(dbeta) <= 16u.  Derived, not measured: the kernel's sums are fp64, so what is left is, per dx element,
        dz = dy * slope                                   1 rounding
        ga * dz                                           1
        ... - m1                                          1, plus the rounding of m1 to fp32
        xh = (x - mean) * rstd                            2
        m2 to fp32                                        1, plus 3 from dz and xh inside its sum; times |xh|
        fma(-xh, m2, .)                                   1
        rstd * t                                          1
    each a relative error u of a term that S_dx contains (times rstd): at most 8u S_dx in first order.  dgamma's
    summands dz xh carry 3 roundings and the result 1: 4u S; dbeta's 1 and 1: 2u S.  16u leaves a factor of 2 and
    is the FLOOR of ``test_nn_grad_gpu``.

(c) Unconditionally, against the true fp64 reference, per element
        |dx - dx64| <= 16u S_dx + rstd^2 (|m2| + |xh| |m1|) 4u max|x| + 4u (|dx| + 2 rstd |xh m2|)
    which is (b) plus the first-order propagation of the tolerances of (a): dx = rstd (ga dz - m1 - xh m2) depends
    on mean only through xh, d xh / d mean = -rstd and d m2 / d mean = -rstd m1, so d dx / d mean =
    rstd^2 (m2 + xh m1); xh and m2 are each proportional to rstd, so a relative change e of rstd changes dx by
    e (dx - 2 rstd xh m2).  In the same way, with dgamma_b, dbeta_b the per-sample sums,
        |dgamma[c] - dgamma64[c]| <= 16u S_dgamma[c] + sum_b (rstd_b |dbeta_b[b, c]| 4u max|x_b| + 4u |dgamma_b[b, c]|)
        |dbeta[c] - dbeta64[c]|   <= 16u S_dbeta[c]            (dbeta does not depend on the statistics).
    Printed per case: the kernel's worst error / bound (asserted <= 1) and the same figure for the framework's fp32
    CUDA backward on the same input (not asserted: its ds, db are formed around zero, and it is expected to exceed
    1 where |mean| >> std).  DESIGN.md records the printed figures.

The side of the kink: the kernel reads it off the forward's fp32 y, the reference off the fp64 z.
``cases.gn_case_kind`` asserts on the CPU that every |z| >= max(KINK, 2 E), E the bound on the forward's
pre-activation error at the element, so the two cannot disagree.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_grad_cases as cases
import nn_grad_pyref as ref
import test_nn_grad_gpu as G
import test_nn_grad_half_gpu as H
from test_nn_half_gpu import DTYPES, to_dev, ulp, widen

from aind_exaspim_image_compression import _native, inference

pytestmark = pytest.mark.gpu
U = cases.U
B_TOL = 16 * U
SLOPES = [0.01, 1.0]


# ---- the three assertions -----------------------------------------------------------------------------------
def sample_max(x):
    """max |x| of each sample, shaped to broadcast against x."""
    return np.abs(x).reshape(x.shape[0], -1).max(axis=1).astype(np.float64).reshape(-1, *(1,) * (x.ndim - 1))


def excess(got, want, bound, kernel=True):
    """max |got - want| / bound; where the bound is 0 the kernel must be exact (the framework is left out there,
    and a non-finite value of the framework is reported as inf)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        assert not kernel, "non-finite gradient"
        return float("inf")
    err = np.abs(got - want)
    pos = bound > 0
    assert not kernel or np.all(err[~pos] == 0)
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check_stats(tag, x, rt, stats):
    """(a).  ``stats``: [b, g, 2] from the device; ``rt``: the true fp64 reference, whose statistics are
    ``nn_pyref.group_norm_parts``'s."""
    mean, rstd = rt["mean"], rt["rstd"]
    got = np.asarray(stats, dtype=np.float64)
    assert np.isfinite(got).all()
    r_mean = float((np.abs(got[..., 0] - mean) / (4 * U * sample_max(x).reshape(-1, 1))).max())
    r_rstd = float((np.abs(got[..., 1] - rstd) / (4 * U * rstd)).max())
    print(f"{tag} (a): mean error {r_mean:.3f} x its tolerance, rstd error {r_rstd:.3f} x its tolerance")
    assert r_mean <= 1.0 and r_rstd <= 1.0, (tag, r_mean, r_rstd)


def bounds_c(rt, x):
    """The per-element bounds of (c) from the true fp64 reference ``rt``."""
    B, C = x.shape[0], x.shape[-1]
    cpg = C // rt["rstd"].shape[1]
    xm = sample_max(x)
    per = lambda m: np.repeat(m, cpg, axis=1).reshape(B, *(1,) * (x.ndim - 2), C)   # noqa: E731  [b, g] -> x's
    rstd, m1, m2, xh = per(rt["rstd"]), per(rt["m1"]), per(rt["m2"]), rt["xh"]
    b_dx = (B_TOL * rt["S_dx"] + rstd ** 2 * (np.abs(m2) + np.abs(xh) * np.abs(m1)) * 4 * U * xm
            + 4 * U * (np.abs(rt["dx"]) + 2 * rstd * np.abs(xh * m2)))
    rstd_c = np.repeat(rt["rstd"], cpg, axis=1)                                      # [b, c]
    b_dg = B_TOL * rt["S_dgamma"] + (rstd_c * np.abs(rt["dbeta_b"]) * 4 * U * xm.reshape(B, 1)
                                     + 4 * U * np.abs(rt["dgamma_b"])).sum(axis=0)
    return b_dx, b_dg, B_TOL * rt["S_dbeta"]


def check_gn(tag, x, dy, gamma, beta, groups, slope, stats, dx, dg, db, framework=None):
    """(a), (b), (c) on what the device returned (numpy).  ``framework``: its (dx, dgamma, dbeta), measured under
    (c) and printed.  Returns the true and the conditional reference and the printed ratios."""
    rt = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope)
    check_stats(tag, x, rt, stats)
    rc = ref.group_norm_lrelu_backward(x, dy, groups, gamma, beta, 1e-5, slope, stats=(stats[..., 0], stats[..., 1]))
    mb = [G.measure(got, rc[k], rc["S_" + k]) for k, got in (("dx", dx), ("dgamma", dg), ("dbeta", db))]
    print(f"{tag} (b): dx {mb[0] / U:.3f} u, dgamma {mb[1] / U:.3f} u, dbeta {mb[2] / U:.3f} u")
    assert max(mb) <= B_TOL, (tag, [m / U for m in mb])
    bnd = bounds_c(rt, x)
    ours = [excess(got, rt[k], b) for k, got, b in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), bnd)]
    line = f"{tag} (c): kernel dx {ours[0]:.3f} dgamma {ours[1]:.3f} dbeta {ours[2]:.3f} x bound"
    theirs = None
    if framework is not None:
        theirs = [excess(got, rt[k], b, kernel=False) for k, got, b in zip(("dx", "dgamma", "dbeta"), framework, bnd)]
        line += f"; framework dx {theirs[0]:.3g} dgamma {theirs[1]:.3g} dbeta {theirs[2]:.3g} x bound"
    print(line)
    assert max(ours) <= 1.0, (tag, ours)
    return rt, rc, ours, theirs


def device_gn(ctx, x, dy, gamma, beta, groups, slope):
    """Training forward and backward in fp32; the device tensors are kept for a second launch."""
    t = {"x": G.dev(x), "dy": G.dev(dy), "gamma": G.dev(gamma), "beta": G.dev(beta)}
    t["y"], t["stats"] = G.gn_forward(ctx, t["x"], groups, t["gamma"], t["beta"], slope)
    t["dx"] = torch.full_like(t["x"], np.nan)
    t["dg"], t["db"] = G.gn_backward(ctx, t["x"], t["y"], t["dy"], t["dx"], groups, t["gamma"], t["stats"], slope)
    return t


def host(t):
    return tuple(t[k].cpu().numpy() for k in ("stats", "dx", "dg", "db"))


def framework_gn(x, dy, gamma, beta, groups, slope):
    xt = G.dev_ncdhw(x, grad=True)
    wt, bt = G.dev(gamma).requires_grad_(True), G.dev(beta).requires_grad_(True)
    F.leaky_relu(F.group_norm(xt, groups, wt, bt, 1e-5), slope).backward(G.dev_ncdhw(dy))
    return G.host_ndhwc(xt.grad), wt.grad.cpu().numpy(), bt.grad.cpu().numpy()


def run_kind(ctx, tag, kind, shape, groups, slope, seed, framework=True):
    x, dy, gamma, beta = cases.gn_case_kind(kind, shape, groups, slope, seed)       # asserts |z| >= max(KINK, 2E)
    t = device_gn(ctx, x, dy, gamma, beta, groups, slope)
    fw = framework_gn(x, dy, gamma, beta, groups, slope) if framework else None
    out = check_gn(tag, x, dy, gamma, beta, groups, slope, *host(t), framework=fw)
    return (x, dy, gamma, beta), t, out


def same_bits(a, b):
    return torch.equal(H.bits(a), H.bits(b))


# ---- 1. the eight distributions -----------------------------------------------------------------------------
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind", cases.GN_KINDS)
def test_groupnorm_backward_distributions(ctx, kind, slope):
    shape, groups = (2, 16, 16, 16, 32), 8
    (x, dy, gamma, beta), t, (rt, rc, _, _) = run_kind(ctx, f"gn {kind} slope={slope}", kind, shape, groups, slope,
                                                       seed=50 + cases.GN_KINDS.index(kind))
    if kind == "constant":
        # xh is exactly 0 (the fp32 mean is the constant): dgamma is exactly 0 and dx = rstd (gamma dz - m1)
        stats, dx, dg, _ = host(t)
        assert np.all(rc["S_dgamma"] == 0) and np.all(dg == 0)
        dz = dy.astype(np.float64) * np.where(rt["z"] > 0, 1.0, slope)
        cpg = shape[-1] // groups
        per = lambda m: np.repeat(m, cpg, axis=1).reshape(shape[0], 1, 1, 1, shape[-1])   # noqa: E731
        want = per(stats[..., 1].astype(np.float64)) * (gamma.astype(np.float64) * dz - per(rc["m1"]))
        assert np.all(np.abs(dx - want) <= B_TOL * rc["S_dx"])


# ---- 2. the U-Net's GroupNorm layers ------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", cases.GN_LAYERS)
def test_groupnorm_backward_layer_table(ctx, c, n):
    """Sample 0 today's input, sample 1 mean 100 with std 1, as in the forward's layer-table test; 32 @ 64^3 holds
    the one sample of mean 100 (8.4 M elements)."""
    kinds = ["mean100"] if (c, n) == (32, 64) else ["today", "mean100"]
    run_kind(ctx, f"gn layer {c}@{n}^3", kinds, (len(kinds), n, n, n, c), 8, 0.01, seed=60 + c + n)


# ---- 3. past the launch caps --------------------------------------------------------------------------------
def cycle_kinds(batch):
    return [cases.GN_KINDS[i % len(cases.GN_KINDS)] for i in range(batch)]


# The launcher (launch_groupnorm_lrelu_bwd_ndhwc, gn_grad_plan), which these shapes are chosen against:
#   apply: at most ceil(8192 / batch) workgroups of 256 threads per sample, a thread moves 4 channels;
#   plan:  nchunk = min(ceil(1024 / batch), spatial / (2 rows_per_iter), 64), rows_per_iter = 256 / (C / 4).
# (64, 16^3, 64): a sample has 4096 * 16 = 65536 four-channel lanes = 256 workgroups against a cap of
#   8192 / 64 = 128, so every thread runs its loop twice; rows_per_iter = 16, spatial / (2 * 16) = 128, and
#   1024 / 64 = 16 binds below it.
# (1100, 2^3, 8): batch > 1024 gives nchunk = 1 (ceil(1024 / 1100) = 1; spatial / (2 * 128) = 0 is raised to 1)
#   and an apply cap of ceil(8192 / 1100) = 8 workgroups, of which the sample's 16 lanes need one.
CAP_SHAPES = [((64, 16, 16, 16, 64), 8), ((1100, 2, 2, 2, 8), 2)]


@pytest.mark.parametrize("shape,groups", CAP_SHAPES)
def test_groupnorm_backward_past_the_launch_cap(ctx, shape, groups):
    """The samples cycle through the eight distributions; (a), (b), (c) on all of them, dgamma / dbeta over the
    whole batch, and a second launch gives the same bits.  Update the comment above and these shapes together with
    the launcher's constants."""
    (x, _, _, _), t, _ = run_kind(ctx, f"gn cap {shape}", cycle_kinds(shape[0]), shape, groups, 0.01, seed=70,
                                  framework=False)
    dx2 = torch.full_like(t["dx"], np.nan)
    dg2, db2 = G.gn_backward(ctx, t["x"], t["y"], t["dy"], dx2, groups, t["gamma"], t["stats"], 0.01)
    assert same_bits(t["dx"], dx2) and same_bits(t["dg"], dg2) and same_bits(t["db"], db2)
    assert torch.equal(t["x"], G.dev(x))                                            # the input is read only


# ---- 4. dead channels ---------------------------------------------------------------------------------------
def test_groupnorm_backward_dead_channels(ctx):
    """gamma[c] = 0 (weight decay) makes z = beta[c]; with beta[c] = +-0 the output is a zero and the side the
    kernel reads off ``y > 0`` is the slope's: dbeta[c] = slope * sum dy -- the one place where the convention at
    the kink itself shows.  Single dead channels in live groups and one group dead altogether (its dx is exactly
    0: S_dx is)."""
    shape, groups, slope = (2, 3, 5, 7, 32), 8, 0.2
    rng = np.random.default_rng(80)
    gamma = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    gamma[::2] *= -1
    beta = (rng.uniform(0.1, 0.5, 32) * rng.choice([-1.0, 1.0], 32)).astype(np.float32)
    dead = {1: 0.3, 6: -0.3, 9: 0.0, 14: -0.0, 28: 0.3, 29: -0.3, 30: 0.0, 31: -0.0}
    for c, v in dead.items():
        gamma[c], beta[c] = 0.0, v
    zero = [c for c, v in dead.items() if v == 0]
    assert np.signbit(beta[14]) and not np.signbit(beta[9])
    x, dy, gamma, beta = cases.gn_case_kind("today", shape, groups, slope, 81, gamma=gamma, beta=beta,
                                            exact_zero=zero)
    t = device_gn(ctx, x, dy, gamma, beta, groups, slope)
    fw = framework_gn(x, dy, gamma, beta, groups, slope)
    stats, dx, dg, db = host(t)
    rt, rc, _, _ = check_gn("gn dead channels", x, dy, gamma, beta, groups, slope, stats, dx, dg, db, framework=fw)
    y = t["y"].cpu().numpy()
    assert np.all(y[..., zero] == 0)
    sdy, sabs = dy.astype(np.float64).sum(axis=(0, 1, 2, 3)), np.abs(dy.astype(np.float64)).sum(axis=(0, 1, 2, 3))
    for c in zero:                                                                  # the slope's side, ours and theirs
        assert abs(db[c] - slope * sdy[c]) <= B_TOL * slope * sabs[c]
        assert abs(fw[2][c] - slope * sdy[c]) <= 4 * B_TOL * slope * sabs[c]
    for c, v in dead.items():
        if v != 0:
            side = 1.0 if v > 0 else slope
            assert abs(db[c] - side * sdy[c]) <= B_TOL * side * sabs[c]
    assert np.all(dx[..., 28:32] == 0)
    G.judge("gn dead channels dbeta", G.measure(db, rt["dbeta"], rt["S_dbeta"]),
            G.measure(fw[2], rt["dbeta"], rt["S_dbeta"], kernel=False))


# ---- 5. non-finite data -------------------------------------------------------------------------------------
def non_finite_case(ctx, dtype, bad, where):
    """One bad element at (sample 1, channel 13) of (2, 3, 5, 7, 32), G = 8: group 3 = channels 12..15.  This is
    data: the kernels compute on it as on any other.

    What the framework's NCDHW backward shares: a bad x makes the group's rstd NaN, so its dx of the (sample, group)
    and its dgamma[12:16] are NaN there too, and its dbeta (a sum of dz alone, the side read off a NaN
    pre-activation: the slope's) stays finite as ours does.  A bad dy reaches the framework's dbeta[13] and
    dgamma[13] and the whole (sample, group) of dx through the two means, as here."""
    shape, groups, slope = (2, 3, 5, 7, 32), 8, 0.01
    code = inference._NATIVE_DTYPES[dtype]
    if dtype == torch.float32:
        x, dy, gamma, beta = cases.gn_case_kind("today", shape, groups, slope, 90)
    else:
        x, dy, gamma, beta = half_case(dtype, "today", shape, groups, slope, 90)
    xb, dyb = x.copy(), dy.copy()
    (xb if where == "x" else dyb)[1, 1, 2, 3, 13] = bad
    g_dev, b_dev = H.f32_dev(gamma), H.f32_dev(beta)
    out = []
    for xi, di in ((x, dy), (xb, dyb)):
        x_t, dy_t = to_dev(xi, dtype), to_dev(di, dtype)
        y_t, stats = H.gn_forward(ctx, x_t, groups, g_dev, b_dev, slope, code)
        dx = torch.full_like(x_t, np.nan)
        dg, db = H.gn_backward(ctx, x_t, y_t, dy_t, dx, groups, g_dev, stats, slope, code)
        out.append((widen(dx), dg.cpu().numpy(), db.cpu().numpy(), stats.cpu().numpy(), widen(y_t)))
    (dx0, dg0, db0, st0, y0), (dx1, dg1, db1, st1, _) = out
    assert all(np.isfinite(a).all() for a in (dx0, dg0, db0, st0))
    bits = lambda a: a.view(np.int32)                                               # noqa: E731
    hit = np.zeros(shape, dtype=bool)
    hit[1, ..., 12:16] = True
    in_group = np.zeros(32, dtype=bool)
    in_group[12:16] = True
    assert np.array_equal(bits(dx1[~hit]), bits(dx0[~hit]))
    assert np.array_equal(bits(dg1[~in_group]), bits(dg0[~in_group]))
    assert np.array_equal(bits(db1[~in_group]), bits(db0[~in_group]))
    if where == "dy":
        assert np.array_equal(bits(st1), bits(st0))
        assert not np.isfinite(dx1[hit]).any()
        assert not np.isfinite(dg1[13]) and not np.isfinite(db1[13])
        rest = [12, 14, 15]
        assert np.array_equal(bits(dg1[rest]), bits(dg0[rest])) and np.array_equal(bits(db1[rest]), bits(db0[rest]))
    else:
        # the forward's statistics of the group: rstd NaN, the mean NaN or the infinity itself
        assert np.isnan(st1[1, 3, 1]) and (np.isnan(st1[1, 3, 0]) or st1[1, 3, 0] == bad)
        keep = np.ones((2, 8), dtype=bool)
        keep[1, 3] = False
        assert np.array_equal(bits(st1[keep]), bits(st0[keep]))
        assert np.isnan(dx1[hit]).all() and np.isnan(dg1[12:16]).all()
        # dbeta: the group's y is NaN, so sample 1 takes the slope's side throughout; a channel whose clean y was
        # nowhere positive in sample 1 keeps its bits, the others are that sum to rounding
        d64 = dy.astype(np.float64)
        side = np.where(y0 > 0, 1.0, slope)
        side[1, ..., 12:16] = slope
        want, s = (d64 * side).sum(axis=(0, 1, 2, 3)), np.abs(d64 * side).sum(axis=(0, 1, 2, 3))
        assert np.isfinite(db1).all()
        assert np.all(np.abs(db1[12:16] - want[12:16]) <= B_TOL * s[12:16])
        unchanged = in_group & ~(y0[1] > 0).any(axis=(0, 1, 2))
        assert np.array_equal(bits(db1[unchanged]), bits(db0[unchanged]))


@pytest.mark.parametrize("where", ["x", "dy"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_groupnorm_backward_non_finite(ctx, bad, where):
    non_finite_case(ctx, torch.float32, bad, where)


# ---- 6. pool and up-sampling at the U-Net's layers ------------------------------------------------------------
@pytest.mark.parametrize("kind,c,n", [("pool", c, n) for c, n in cases.POOL_LAYERS]
                         + [("up", c, n) for c, n in cases.UP_LAYERS])
def test_pool_and_upsample_backward_layer_table(ctx, kind, c, n):
    """Batch 2; batch 1 for the two largest (32 @ 64^3 pooled, 32 @ 32^3 up-sampled to 64^3)."""
    if kind == "pool":
        shape = (1 if (c, n) == (32, 64) else 2, n, n, n, c)
        G.pool_check(ctx, np.random.default_rng(c + n).standard_normal(shape).astype(np.float32), c)
    else:
        G.up_check(ctx, (1 if (c, n) == (32, 32) else 2, n, n, n, c))


# ---- 7. the autograd wrappers -------------------------------------------------------------------------------
def ndhwc_leaf(a):
    """numpy [b, d, h, w, c] -> a [b, c, d, h, w] leaf on NDHWC memory that requires a gradient."""
    return G.dev(a).permute(0, 4, 1, 2, 3).requires_grad_(True)


def grad_forms(make_y, x_host):
    """d(make_y(x)) / dx for one gradient handed over in four forms -- dense NDHWC fp32, NCDHW-contiguous, float64
    and, for the gradient of ones, the expanded stride-0 tensor of ``y.sum().backward()`` -- must be the same
    bits; the input is bit-unchanged by forward and backward.  Returns the dense form's (x.grad, gradient)."""
    x = ndhwc_leaf(x_host)
    x0 = x.detach().clone()
    with torch.enable_grad():
        y = make_y(x)
    assert y.is_contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(H.bits(x.detach()), H.bits(x0))
    g = torch.randn(y.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) \
        .contiguous(memory_format=torch.channels_last_3d)
    dense, = torch.autograd.grad(y, x, g, retain_graph=True)
    ncdhw = g.contiguous()
    assert not ncdhw.is_contiguous(memory_format=torch.channels_last_3d) or min(y.shape[1:]) == 1
    other, = torch.autograd.grad(y, x, ncdhw, retain_graph=True)
    assert same_bits(dense, other)
    other, = torch.autograd.grad(y, x, g.double(), retain_graph=True)
    assert other.dtype == torch.float32 and same_bits(dense, other)
    ones, = torch.autograd.grad(y, x, torch.ones_like(g), retain_graph=True)
    y.sum().backward()
    assert same_bits(ones, x.grad)
    assert torch.equal(H.bits(x.detach()), H.bits(x0))
    return dense, g


def test_autograd_wrappers(ctx):
    shape, groups, slope = (2, 3, 5, 7, 32), 8, 0.01
    x_gn, _, gamma, beta = cases.gn_case_kind("today", shape, groups, slope, 95)
    norm = torch.nn.GroupNorm(groups, 32).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy(gamma))
        norm.bias.copy_(torch.from_numpy(beta))
    mod = inference.FusedGroupNormLeakyReLU(norm, torch.nn.LeakyReLU(slope), inplace=False, trainable=True)

    def gn(x):
        y = mod(x)
        assert type(y.grad_fn).__name__ == "_GroupNormLeakyReLUFnBackward"
        return y

    # (ii), (iii) with trainable parameters
    dense, g = grad_forms(gn, x_gn)
    norm.weight.grad = norm.bias.grad = None
    x = ndhwc_leaf(x_gn)
    with torch.enable_grad():
        gn(x).backward(g)
    assert same_bits(x.grad, dense)
    dg, db = norm.weight.grad.clone(), norm.bias.grad.clone()
    r = ref.group_norm_lrelu_backward(x_gn, G.host_ndhwc(g), groups, gamma, beta, 1e-5, slope)
    fw = framework_gn(x_gn, G.host_ndhwc(g), gamma, beta, groups, slope)
    for k, ours, theirs in (("dx", G.host_ndhwc(dense), fw[0]), ("dgamma", dg.cpu().numpy(), fw[1]),
                            ("dbeta", db.cpu().numpy(), fw[2])):
        G.judge("wrapper gn " + k, G.measure(ours, r[k], r["S_" + k]), G.measure(theirs, r[k], r["S_" + k], kernel=False))
    # (i) frozen affine parameters: still the native Function, the same dx, no parameter gradient
    norm.weight.grad = norm.bias.grad = None
    norm.weight.requires_grad_(False)
    norm.bias.requires_grad_(False)
    frozen, _ = grad_forms(gn, x_gn)
    assert same_bits(frozen, dense)
    assert norm.weight.grad is None and norm.bias.grad is None

    # the resampling modules
    pool = inference._ResampleNDHWC(torch.nn.MaxPool3d(2), trainable=True)
    up = inference._ResampleNDHWC(torch.nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
                                  trainable=True)

    def named(m, name):
        def f(x):
            y = m(x)
            assert type(y.grad_fn).__name__ == name
            return y
        return f

    xp = np.random.default_rng(96).standard_normal((2, 5, 4, 6, 8)).astype(np.float32)
    dense, g = grad_forms(named(pool, "_MaxPool2FnBackward"), xp)
    xt = G.dev_ncdhw(xp, grad=True)
    F.max_pool3d(xt, 2).backward(g.contiguous())
    assert torch.equal(dense, xt.grad)
    dense, g = grad_forms(named(up, "_Upsample2FnBackward"), xp)
    want, s = ref.upsample2_trilinear_backward(G.host_ndhwc(g))
    xt = G.dev_ncdhw(xp, grad=True)
    F.interpolate(xt, scale_factor=2, mode="trilinear", align_corners=True).backward(g.contiguous())
    G.judge("wrapper up dx", G.measure(G.host_ndhwc(dense), want, s), G.measure(G.host_ndhwc(xt.grad), want, s, kernel=False))


# ---- 8. half precision: one case per family 1, 3 and 5 --------------------------------------------------------
# fp16 cannot hold mean1000 with a spread (its spacing at 1000 is 0.5, bf16's is 4), so the amplifying kinds here
# are mean100 and std1e-2, for both types.
_half_inputs = {}


def half_case(dtype, kind, shape, groups, slope, seed):
    """``cases.gn_case_kind`` on x, dy rounded to ``dtype`` (fp32 arrays of half values), built once per case."""
    key = (dtype, str(kind), shape, groups, slope, seed)
    if key not in _half_inputs:
        _half_inputs[key] = cases.gn_case_kind(kind, shape, groups, slope, seed,
                                               storage=(lambda a: H.round_to(a, dtype), lambda a: ulp(a, dtype)))
    return _half_inputs[key]


def half_gn_check(ctx, name, tag, kind, shape, groups, slope, seed):
    """Conditions A and B of ``test_nn_grad_half_gpu`` and, on the fp32 entry's results A ties the half kernel to,
    (a), (b), (c) with the half forward's statistics."""
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    x, dy, gamma, beta = half_case(dtype, kind, shape, groups, slope, seed)
    x_t, dy_t = to_dev(x, dtype), to_dev(dy, dtype)
    assert np.array_equal(widen(x_t), x) and np.array_equal(widen(dy_t), dy)
    g_dev, b_dev = H.f32_dev(gamma), H.f32_dev(beta)
    y_t, stats = H.gn_forward(ctx, x_t, groups, g_dev, b_dev, slope, code)
    dx_t = torch.full_like(x_t, np.nan)
    dg, db = H.gn_backward(ctx, x_t, y_t, dy_t, dx_t, groups, g_dev, stats, slope, code)
    # A: the fp32 entry on the widened x, y, dy with the same (mean, rstd)
    dx32 = torch.full_like(x_t, np.nan, dtype=torch.float32)
    dg32, db32 = H.gn_backward(ctx, x_t.float(), y_t.float(), dy_t.float(), dx32, groups, g_dev, stats, slope,
                               _native.DTYPE_F32)
    assert same_bits(dx_t, dx32.to(dtype)) and same_bits(dg, dg32) and same_bits(db, db32)
    rt, _, _, _ = check_gn(f"{tag} {name} (fp32 entry on the half values)", x, dy, gamma, beta, groups, slope,
                           stats.cpu().numpy(), widen(dx32), dg32.cpu().numpy(), db32.cpu().numpy())
    # B: against fp64
    got = widen(dx_t)
    assert np.isfinite(got).all()
    bound, m32 = H.bound_b(rt["dx"], rt["S_dx"], widen(dx32), dtype)
    over = float((np.abs(got.astype(np.float64) - rt["dx"]) / bound).max())
    print(f"{tag} {name}: m32 {m32 / U:.3f} u, half kernel {over:.3f} x bound")
    assert over <= 1.0, (tag, name, over)
    dx2 = torch.full_like(x_t, np.nan)
    dg2, db2 = H.gn_backward(ctx, x_t, y_t, dy_t, dx2, groups, g_dev, stats, slope, code)
    assert same_bits(dx_t, dx2) and same_bits(dg, dg2) and same_bits(db, db2)


@pytest.mark.parametrize("kind", ["mean100", "std1e-2"])
@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_backward_distributions_half(ctx, name, kind):
    half_gn_check(ctx, name, f"gn {kind}", kind, (2, 16, 16, 16, 32), 8, 0.01, 50)


@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_backward_past_the_launch_cap_half(ctx, name):
    """(40, 16^3, 64): the apply cap is ceil(8192 / 40) = 205 workgroups against the 256 a sample needs, so the
    threads of the first 51 run their loop twice and the others once; the plan has ceil(1024 / 40) = 26 chunks."""
    kinds = ["today", "mean10", "mean100", "std1e-2", "constant"]
    shape = (40, 16, 16, 16, 64)
    half_gn_check(ctx, name, "gn cap", [kinds[i % len(kinds)] for i in range(shape[0])], shape, 8, 0.01, 70)


@pytest.mark.parametrize("name", DTYPES)
def test_groupnorm_backward_non_finite_half(ctx, name):
    non_finite_case(ctx, DTYPES[name], np.nan, "x")
