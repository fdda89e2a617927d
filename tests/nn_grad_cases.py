"""Shapes and input builders shared by the CPU and GPU tests of the training kernels ([b, d, h, w, c])."""
import numpy as np

import nn_pyref

GN_CASES = [((2, 3, 5, 7, 32), 8), ((1, 1, 1, 1, 4), 1), ((3, 4, 4, 4, 1024), 32), ((2, 16, 16, 16, 64), 8),
            ((5, 2, 3, 2, 8), 2), ((1, 64, 64, 64, 32), 8)]
POOL_SHAPES = [(1, 7, 5, 9, 4), (3, 2, 3, 2, 8), (2, 4, 4, 4, 1024), (1, 65, 3, 33, 12)]
UP_SHAPES = [(1, 1, 1, 1, 4), (2, 1, 3, 2, 4), (1, 5, 7, 3, 8), (3, 4, 4, 4, 1024), (1, 32, 32, 32, 32)]
KINK = 1e-3


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
