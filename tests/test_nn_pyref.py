"""Reference hygiene for ``nn_pyref.py`` (the fp64 restatement the BM4DNet stage's NDHWC kernels are tested
against): it has to equal torch's CPU float64 functional ops -- values to rounding, NaN / inf placement and
the max-pool's selected bit patterns exactly.  CPU, a few seconds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_pyref as R


def ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def ndhwc(t):
    return np.moveaxis(t.numpy(), 1, -1)


def rand(shape, seed, scale=1.0, loc=0.0):
    return np.random.default_rng(seed).standard_normal(shape) * scale + loc


@pytest.mark.parametrize("shape,groups", [((2, 3, 5, 4, 16), 4), ((1, 1, 1, 1, 8), 2), ((3, 7, 1, 3, 32), 8),
                                          ((2, 2, 3, 5, 12), 3)])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("slope", [0.01, 0.2, 1.0])
def test_group_norm_lrelu_matches_torch(shape, groups, affine, slope):
    c = shape[-1]
    x = rand(shape, c + groups, 2.0, 10.0)
    cb = rand(c, 1, 5.0)
    gamma, beta = (rand(c, 2), rand(c, 3)) if affine else (None, None)
    got = R.group_norm_lrelu(x, groups, gamma, beta, 1e-5, slope, cb)
    t = ncdhw(x) + torch.from_numpy(cb).view(1, -1, 1, 1, 1)
    want = F.leaky_relu(F.group_norm(t, groups, None if gamma is None else torch.from_numpy(gamma),
                                     None if beta is None else torch.from_numpy(beta), 1e-5), slope)
    np.testing.assert_allclose(got, ndhwc(want), rtol=1e-12, atol=1e-12)
    mean, var, a, z = R.group_norm_parts(x, groups, gamma, beta, 1e-5, cb)
    assert mean.shape == var.shape == (shape[0], groups) and a.shape == (shape[0], c) and z.shape == x.shape


def test_group_norm_constant_and_spread_groups():
    x = np.full((2, 4, 3, 2, 8), np.float32(5.3), np.float64)      # a float32 value: its sums are exact
    x[1, ..., 4:] = rand((4, 3, 2, 4), 0, 1e-3, 1.0)          # sample 1, group 1: mean 1, std 1e-3
    x[0, ..., 4:] += np.arange(4) * 1000.0                     # channels of one group far apart
    gamma, beta = rand(8, 1), rand(8, 2)
    got = R.group_norm_lrelu(x, 2, gamma, beta, 1e-5, 0.2)
    want = F.leaky_relu(F.group_norm(ncdhw(x), 2, torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5), 0.2)
    np.testing.assert_allclose(got, ndhwc(want), rtol=1e-10, atol=1e-10)
    _, var, _, z = R.group_norm_parts(x, 2, gamma, beta)
    assert var[0, 0] == 0.0 and np.all(z[0, ..., :4] == beta[:4])          # a constant group: exactly beta


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_group_norm_non_finite_poisons_its_group_only(bad):
    x = rand((2, 3, 4, 2, 16), 5)
    x[1, 2, 1, 0, 9] = bad                                     # sample 1, group 2 of 4
    got = R.group_norm_lrelu(x, 4, rand(16, 6), rand(16, 7), 1e-5, 0.01)
    want = ndhwc(F.leaky_relu(F.group_norm(ncdhw(x), 4, torch.from_numpy(rand(16, 6)),
                                           torch.from_numpy(rand(16, 7)), 1e-5), 0.01))
    bad_mask = np.zeros(x.shape, bool)
    bad_mask[1, ..., 8:12] = True
    assert np.all(np.isnan(got[bad_mask])) and np.all(np.isfinite(got[~bad_mask]))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))       # the framework agrees: NaN, not -inf
    np.testing.assert_allclose(got[~bad_mask], want[~bad_mask], rtol=1e-12, atol=1e-12)


def test_leaky_relu_signs():
    z = np.array([-0.0, 0.0, -1.5, 2.0, np.nan, -np.inf, np.inf])
    got = R.leaky_relu(z, 0.01)
    want = F.leaky_relu(torch.from_numpy(z), 0.01).numpy()
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def _pool_case(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=shape).astype(np.float32)     # many ties
    x[x == 0] = np.where(rng.random(np.count_nonzero(x == 0)) < 0.5, -0.0, 0.0)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 20), replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=idx.size)
    return x


@pytest.mark.parametrize("shape", [(2, 4, 6, 8, 3), (1, 5, 7, 3, 2), (3, 2, 2, 2, 4), (1, 3, 2, 5, 1)])
def test_maxpool2_matches_torch_bit_for_bit(shape):
    x = _pool_case(shape, sum(shape))
    got = R.maxpool2(x)
    want = ndhwc(F.max_pool3d(ncdhw(x), 2))
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    x64 = x.astype(np.float64)
    np.testing.assert_array_equal(R.maxpool2(x64).view(np.int64), ndhwc(F.max_pool3d(ncdhw(x64), 2)).view(np.int64))


def test_maxpool2_nan_in_every_window_position_and_zero_ties():
    x = np.zeros((8, 2, 2, 2, 2), np.float32)
    for k in range(8):
        x[k, k >> 2, (k >> 1) & 1, k & 1, 0] = np.nan
        x[k, ..., 1] = 1.0
        x[k, k >> 2, (k >> 1) & 1, k & 1, 1] = -np.inf
    got = R.maxpool2(x)
    assert np.all(np.isnan(got[..., 0])) and np.all(got[..., 1] == 1.0)
    z = np.full((2, 2, 2, 2, 1), 0.0, np.float32)
    z[0, 0, 0, 0, 0] = -0.0                                    # first position -0: the tie keeps -0
    z[1, 0, 0, 1, 0] = -0.0                                    # first position +0: stays +0
    got = R.maxpool2(z)
    assert np.signbit(got[0, 0, 0, 0, 0]) and not np.signbit(got[1, 0, 0, 0, 0])
    np.testing.assert_array_equal(got.view(np.int32), ndhwc(F.max_pool3d(ncdhw(z), 2)).view(np.int32))


@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 3), (1, 1, 1, 1, 2), (1, 1, 4, 2, 1), (2, 5, 1, 3, 2),
                                   (1, 4, 4, 4, 4)])
def test_upsample2_matches_torch(shape):
    x = rand(shape, sum(shape), 3.0)
    got = R.upsample2_trilinear(x)
    want = ndhwc(F.interpolate(ncdhw(x), scale_factor=2, mode="trilinear", align_corners=True))
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)
    # the corners of an align-corners interpolation are the input's corners
    np.testing.assert_array_equal(got[:, [0, -1]][:, :, [0, -1]][:, :, :, [0, -1]],
                                  x[:, [0, -1]][:, :, [0, -1]][:, :, :, [0, -1]])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_upsample2_non_finite_masks_match_torch(bad):
    x = rand((2, 3, 4, 5, 2), 11)
    x[0, 1, 2, 3, 0] = bad
    x[1, 2, 3, 4, 1] = bad                                     # on the far corner
    x[1, 0, 0, 0, 0] = -bad if bad == bad else bad             # opposite infinities meet in one output
    x[1, 0, 0, 1, 0] = bad
    got = R.upsample2_trilinear(x)
    want = ndhwc(F.interpolate(ncdhw(x), scale_factor=2, mode="trilinear", align_corners=True))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.count_nonzero(~fin) > 0
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-13, atol=1e-13)
