"""Shapes and input builders shared by the CPU and GPU tests of the training kernels ([b, d, h, w, c])."""
import numpy as np

import nn_pyref

GN_CASES = [((2, 3, 5, 7, 32), 8), ((1, 1, 1, 1, 4), 1), ((3, 4, 4, 4, 1024), 32), ((2, 16, 16, 16, 64), 8),
            ((5, 2, 3, 2, 8), 2), ((1, 64, 64, 64, 32), 8)]
POOL_SHAPES = [(1, 7, 5, 9, 4), (3, 2, 3, 2, 8), (2, 4, 4, 4, 1024), (1, 65, 3, 33, 12)]
UP_SHAPES = [(1, 1, 1, 1, 4), (2, 1, 3, 2, 4), (1, 5, 7, 3, 8), (3, 4, 4, 4, 1024), (1, 32, 32, 32, 32)]
KINK = 1e-3
U = 2.0 ** -24                         # fp32 unit round-off

# The U-Net's layers at a 64^3 patch as (channels, extent), checked against unet3d.UNet by
# test_nn_kernels_gpu.test_layer_table.
GN_LAYERS = [(32, 64), (64, 32), (128, 16), (256, 8), (256, 4), (128, 8), (64, 16), (32, 32)]
POOL_LAYERS = [(32, 64), (64, 32), (128, 16), (256, 8)]
UP_LAYERS = [(256, 4), (128, 8), (64, 16), (32, 32)]
GN_KINDS = ["today", "mean10", "mean100", "mean1000", "std1e-2", "std1e-3", "constant", "spread"]


def gn_inputs(kind, shape, groups, seed):
    """Channels-last fp32 data [b, d, h, w, c] of one named distribution (per channel unless said)."""
    rng = np.random.default_rng(seed)
    b, c = shape[0], shape[-1]
    n = rng.standard_normal(shape, dtype=np.float32)
    if kind == "today":
        return n * 3 + 1.5
    if kind.startswith("mean"):                               # mean<m>: m + N(0, 1), mean/std = m
        return n + np.float32(float(kind[4:]))
    if kind.startswith("std"):                                # std<s>: 1 + s N(0, 1)
        return 1 + np.float32(float(kind[3:])) * n
    if kind == "constant":
        return np.full(shape, 5.3, np.float32)
    if kind == "spread":                                      # the channels of a group far apart, each narrow
        return n * 0.5 + (rng.standard_normal(c) * 300).astype(np.float32)
    raise ValueError(kind)


def gn_preact_bound(x, groups, gamma, beta, eps=1e-5, cbias=None):
    """``(z, E)``: the fp64 pre-activation of GroupNorm(x + cbias) and the bound E on the error of the fused fp32
    forward's pre-activation, E = u (4|a mu| + 4|a cb| + 16 (|z| + |beta| + |gamma|)) -- derived in
    ``test_nn_kernels_gpu.gn_bound``, which applies the activation to it."""
    return _preact_parts(x, groups, gamma, beta, eps, cbias)[:2]


def _preact_parts(x, groups, gamma, beta, eps=1e-5, cbias=None):
    """``(z, E, var)`` of ``gn_preact_bound``, var[b, g] the groups' fp64 variance."""
    c = x.shape[-1]
    mean, var, a, z = nn_pyref.group_norm_parts(x, groups, gamma, beta, eps, cbias)
    mu = np.repeat(mean, c // groups, axis=1)                                # [b, c]
    cb = np.zeros(c) if cbias is None else np.abs(np.asarray(cbias, np.float64))
    ga = np.ones(c) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    be = np.zeros(c) if beta is None else np.abs(np.asarray(beta, np.float64))
    lead = (4 * np.abs(a * mu) + 4 * np.abs(a) * cb + 16 * (be + ga)).reshape(x.shape[0], *(1,) * (x.ndim - 2), c)
    return z, U * (lead + 16 * np.abs(z)), var


def gn_case(shape, groups, slope, seed, affine=True, negative_gamma=False):
    """``(x, dy, gamma, beta)`` in fp32.  The one-voxel shape is constant (variance 0).  For slope != 1 the
    elements of x are nudged until every fp64 pre-activation has |z| >= KINK: one sign flip at the kink
    changes a group's sums by far more than rounding, and which side a value within rounding of 0 falls on is
    not something two fp32 evaluations have to agree about."""
    rng = np.random.default_rng(seed)
    C = shape[-1]
    x = (rng.standard_normal(shape) * 1.5 + 0.5).astype(np.float32)
    if int(np.prod(shape[1:4])) == 1 and groups == 1:
        x[:] = np.float32(1.5)
    dy = rng.standard_normal(shape).astype(np.float32)
    gamma = beta = None
    if affine:
        gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
        if negative_gamma:
            gamma[::2] *= -1
        beta = (rng.uniform(0.1, 0.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    if slope != 1.0:
        for _ in range(100):
            z = nn_pyref.group_norm_parts(x, groups, gamma, beta, 1e-5)[3]
            bad = np.abs(z) < KINK
            if not bad.any():
                break
            x[bad] += np.float32(0.03125)
    return x, dy, gamma, beta


def kink_free(x, groups, gamma, beta):
    return bool((np.abs(nn_pyref.group_norm_parts(x, groups, gamma, beta, 1e-5)[3]) >= KINK).all())


def gn_case_kind(kind, shape, groups, slope, seed, gamma=None, beta=None, exact_zero=(), storage=None):
    """``gn_case`` on a named distribution of ``gn_inputs``: ``(x, dy, gamma, beta)`` in fp32, gamma of mixed
    sign.  ``kind``: one name, or one name per sample.  ``gamma``, ``beta``: given instead of drawn.

    The elements of x are nudged until every fp64 pre-activation has |z| >= KINK, for every slope (so the
    slopes of a case share their x).  A nudge is 1/32 of the standard deviation of the element's group -- in
    units of z that is |gamma| / 32 whatever the scale of the data, where a fixed step of 0.03125 is 30 sigma
    for ``std1e-3``.  A constant group (deviation 0) cannot be nudged and does not need it: its z is beta.

    Asserted before returning, so before any GPU call: every element has |z| >= KINK and |z| >= 2 E, E the
    bound on the fp32 forward's pre-activation error at that element (``gn_preact_bound``) -- the forward's y and
    the fp64 z then lie on the same side of the kink, which is what lets a backward that reads the side off y be
    compared with a reference that reads it off z.  (E is below KINK / 2 everywhere but on ``constant``, where
    4u |a mean| reaches 6e-4 while no |z| = |beta| is below 0.1; elements short of 2 E are nudged like those short
    of KINK, and none is exempt.)  ``exact_zero``: channels with gamma = beta = 0, whose z is exactly 0 in any
    arithmetic (E = 0 there, nothing to disagree about); they are required to be exactly that and are the only
    elements excepted.  ``storage = (round, spacing)`` for a half-precision case: x and dy are rounded to the
    storage type (fp32 arrays of half values), every nudge is at least two spacings of the type at the element
    and is rounded again."""
    rng = np.random.default_rng(seed)
    C = shape[-1]
    if isinstance(kind, str):
        x = gn_inputs(kind, shape, groups, seed)
    else:
        assert len(kind) == shape[0]
        x = np.concatenate([gn_inputs(k, (1,) + tuple(shape[1:]), groups, seed + 1 + i) for i, k in enumerate(kind)])
    x = np.ascontiguousarray(x, dtype=np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    if storage is not None:
        x, dy = storage[0](x), storage[0](dy)
    if gamma is None:
        gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
        gamma[::2] *= -1
    if beta is None:
        beta = (rng.uniform(0.1, 0.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    live = np.ones(C, dtype=bool)
    live[list(exact_zero)] = False
    assert np.all(gamma[~live] == 0) and np.all(beta[~live] == 0)
    cpg = C // groups
    for _ in range(100):
        z, E, var = _preact_parts(x, groups, gamma, beta)
        bad = (np.abs(z) < np.maximum(KINK, 2 * E)) & live
        if not bad.any():
            break
        step = np.repeat(np.sqrt(var) / 32, cpg, axis=1).reshape(shape[0], *(1,) * (len(shape) - 2), C)
        step = np.broadcast_to(step, shape)[bad]
        if storage is not None:
            step = np.maximum(step, 2 * storage[1](x[bad]))
        x[bad] += step.astype(np.float32)
        if storage is not None:
            x = storage[0](x)
    assert not bad.any(), (kind, int(np.count_nonzero(bad)), float(E.max()))     # z, E: those of the final x
    assert np.all(z[..., ~live] == 0) and np.all(E[..., ~live] == 0)
    return x, dy, gamma, beta


def pool_tie_input(shape, seed):
    """Values in {-1, -0.0, +0.0, 1}: every window has ties, among them zeros of both signs."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=shape)


def pool_nan_input(seed):
    """(1, 4, 4, 6, 4): twelve windows; window k < 8 has a NaN at position k, window 8 NaNs at positions 2 and
    5, window 9 at 0 and 7, windows 10 and 11 none."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((1, 4, 4, 6, 4)).astype(np.float32)
    wins = [(od, oh, ow) for od in range(2) for oh in range(2) for ow in range(3)]
    plan = [[k] for k in range(8)] + [[2, 5], [0, 7]]
    for (od, oh, ow), ks in zip(wins, plan):
        for k in ks:
            x[0, 2 * od + (k >> 2), 2 * oh + ((k >> 1) & 1), 2 * ow + (k & 1), :] = np.nan
    return x
