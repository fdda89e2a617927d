"""The stage kernels keep a half group's spectrum in the DCT's register pairs: Haar butterflies
through operand-half selectors, details moved to their slots by the shrinkage, the halves' approximations swapped
as they lie.  What that touches, on inputs small enough for a few seconds each, through the staged entry
(exabm4d_stage_dev) and the uint16 pipeline, bit for bit against the oracle: every group size in one volume
(each half-group body, both waves of a pair and the one-block group that is one wave's alone), a coefficient
equal to the hard threshold, details of +0.0 and -0.0, a Wiener group with an all-zero basic spectrum, a tile
with fewer groups than wave pairs, and a batch whose volumes have different numerator units."""
import numpy as np
import pytest

import bm_adversarial_inputs as adv
from util import ctx_options

from aind_exaspim_image_compression import _native

pytestmark = pytest.mark.gpu
SIGMA = 24.0
OFFSET = 37.0
EMPTY = 0xFFFFFFFF


def every_size_volume(shape=(16, 20, 24), seed=0):
    """uint16.  A quiet floor (groups of 16); ramps along x that steepen with y (4 and 8); isolated bright voxels
    whose blocks match nothing (1); and the same bright voxels every 4 columns on a noiseless floor, where a block
    equals its copy 4 columns on and nothing else (2)."""
    rng = np.random.default_rng(seed)
    _, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    v = 300.0 + rng.normal(0, 6.0, shape)
    v += np.where(y >= 10, (y - 9) * 6.0 * x, 0.0)
    hit = (rng.random(shape) < 0.04) & (x >= 12) & (y < 12)
    v[hit] += rng.uniform(3000, 20000, int(hit.sum()))
    lit = rng.random((shape[0], 8, 4)) < 0.08
    amp = np.rint(rng.uniform(3000, 20000, (shape[0], 8, 4)))
    v[:, :8, 12:] = 300.0 + np.tile(np.where(lit, amp, 0.0), (1, 1, (shape[2] - 12) // 4))
    return np.clip(np.rint(v), 0, 65535).astype(np.uint16)


def group_sizes(keys):
    """The K of every group: the largest power of two within its table's length."""
    n = (keys != EMPTY).sum(axis=-1)
    return set((2 ** np.floor(np.log2(np.maximum(n, 1)))).astype(int).ravel().tolist())


def _stage_gpu(ctx, noisy, keys, sigma, basic=None, data_exp=None, params=None):
    bufs = [ctx.to_device(noisy), ctx.to_device(basic) if basic is not None else None, ctx.to_device(keys),
            ctx.alloc(noisy.nbytes).fill(0xFF), ctx.alloc(noisy.nbytes).fill(0xFF)]
    try:
        ctx.stage(bufs[0], bufs[1], bufs[2], noisy.shape, sigma, bufs[3], bufs[4], params=params, data_exp=data_exp)
        ctx.sync()
        return bufs[3].download(noisy.shape, np.float32), bufs[4].download(noisy.shape, np.float32)
    finally:
        for b in bufs:
            if b is not None:
                b.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_stage(ctx, oracle, noisy, keys, sigma=SIGMA, basic=None, data_exp=None, what="", **kw):
    num_w, den_w = oracle.stage(noisy, keys, sigma, basic=basic, data_exp=data_exp, **kw)
    params = _native.default_params(**kw) if kw else None
    num_g, den_g = _stage_gpu(ctx, noisy, keys, sigma, basic=basic, data_exp=data_exp, params=params)
    assert np.array_equal(den_g, den_w), what
    assert np.array_equal(num_g, num_w), what
    assert np.array_equal(_bits(num_g), _bits(num_w)), what + " (sign of a zero)"
    return num_g, den_g


def _u16_gpu(ctx, vol, sigma, offset, stages=2):
    d_in, d_out = ctx.to_device(vol), ctx.alloc(vol.nbytes)
    try:
        ctx.denoise_u16(d_in, d_out, vol.shape, sigma, offset, stages=stages)
        ctx.sync()
        return d_out.download(vol.shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()


@pytest.fixture(scope="module")
def every_size(oracle):
    """(uint16 volume, its fp32 copy, stage-1 tables, stage-1 estimate, stage-2 tables), computed once."""
    vol = every_size_volume()
    f32 = vol.astype(np.float32)
    keys1 = oracle.blockmatch(f32, SIGMA, 3.0)
    basic = oracle.bm4d(f32, SIGMA, stages=1, data_exp=17)
    keys2 = oracle.blockmatch(basic, SIGMA, 0.6)
    for k in (keys1, keys2):
        k.setflags(write=False)
    return vol, f32, keys1, basic, keys2


def test_every_group_size_in_one_volume_hard_threshold_stage(ctx, oracle, every_size):
    _, f32, keys1, _, _ = every_size
    assert group_sizes(keys1) == {1, 2, 4, 8, 16}
    _assert_stage(ctx, oracle, f32, keys1)
    _assert_stage(ctx, oracle, f32, keys1, data_exp=17)


@pytest.mark.parametrize("pairvol", [1, 0])
def test_every_group_size_in_one_volume_wiener_stage(ctx, oracle, every_size, pairvol):
    """With the interleaved (noisy, basic) volume a register pair is one block of both volumes, without it two
    blocks of one: the first Haar level reads either."""
    _, f32, keys1, basic, keys2 = every_size
    assert group_sizes(keys2) == {1, 2, 4, 8, 16}
    with ctx_options(ctx, stage_pairvol=pairvol):
        _assert_stage(ctx, oracle, f32, keys2, basic=basic, data_exp=17)
        _assert_stage(ctx, oracle, f32, keys1, basic=basic)            # other tables will do as well


def test_every_group_size_in_one_volume_uint16_pipeline(ctx, oracle, every_size):
    vol = every_size[0]
    for stages in (1, 2):
        assert np.array_equal(_u16_gpu(ctx, vol, SIGMA, OFFSET, stages), oracle.bm4d_u16(vol, SIGMA, OFFSET, stages=stages))


@pytest.mark.parametrize("lam", [2.0, 1.0])
def test_coefficient_equal_to_the_hard_threshold(ctx, oracle, lam):
    """A constant volume has one non-zero coefficient per group, the approximation of the DC plane, which the two
    waves of a pair form together at the top level; every detail is v + (-v) = +0.0.  At sigma_eq the threshold
    IS that coefficient: it stays, as at the fp32 number below; at the number above the group is shrunk to 0."""
    v, shape = 5.0, (16, 20, 24)
    vol = np.full(shape, v, dtype=np.float32)
    keys = oracle.blockmatch(vol, SIGMA, 3.0)
    assert group_sizes(keys) == {16}
    for i, sigma in enumerate(adv.hard_threshold_sigmas(oracle, v, lam)):
        num, den = _assert_stage(ctx, oracle, vol, keys, sigma=sigma, what=f"sigma {sigma!r}", lambda_ht=lam)
        assert (den > 0).all()
        if i < 2:
            assert np.abs(num / den - v).max() <= 1e-5 * v
        else:
            assert (num == 0).all()


def signed_zero_volume(shape=(16, 20, 24)):
    """fp32.  -0.0 where x < 12, +0.0 beyond, and a slab of counts at high y that sets the numerator's unit: blocks
    of zeros of either sign are at distance 0 from each other, so groups mix them in table order."""
    vol = np.zeros(shape, dtype=np.float32)
    vol[:, :, :12] = -0.0
    rng = np.random.default_rng(3)
    vol[:, 14:, :] = np.rint(rng.normal(500.0, 30.0, vol[:, 14:, :].shape)).astype(np.float32)
    return vol


def test_details_of_either_zero(ctx, oracle):
    """x0 + (-x1) on zeros: (-0) - (+0) = -0.0, (+0) - (-0) = (+0) - (+0) = +0.0.  The oracle's group transform
    shows that the input reaches both; both stages equal the oracle down to the sign of a zero."""
    vol = signed_zero_volume()
    neg, pos = np.full((8, 8, 8), -0.0, np.float32), np.zeros((8, 8, 8), np.float32)
    G = oracle.group_transform(np.stack([neg, pos] * 8))
    details = _bits(G[1:])
    assert (details == 0x80000000).any() and (details == 0).any() and (G == 0).all()
    keys = oracle.blockmatch(vol, SIGMA, 3.0)
    assert 16 in group_sizes(keys)
    _assert_stage(ctx, oracle, vol, keys)
    basic = vol.copy()
    basic[:, 14:, :] += 3.0
    _assert_stage(ctx, oracle, vol, keys, basic=basic)
    _assert_stage(ctx, oracle, vol, keys, basic=-basic)                # a basic estimate of negative counts and zeros


def test_wiener_group_with_an_all_zero_basic_spectrum(ctx, oracle, every_size):
    """basic = 0 on the quiet region: e = 0, so every weight W is 0, the estimate is 0 and the statistic sum W^2
    clamps to 1 -- in groups of every size; elsewhere the basic estimate is the noisy volume."""
    _, f32, keys1, _, _ = every_size
    basic = f32.copy()
    basic[:, :, :12] = 0.0
    _assert_stage(ctx, oracle, f32, keys1, basic=basic, data_exp=17)
    zero = np.zeros_like(f32)
    num, den = _assert_stage(ctx, oracle, f32, keys1, basic=zero, data_exp=17)
    assert (num == 0).all() and (den > 0).all()


def test_edge_tile_with_fewer_groups_than_wave_pairs(ctx, oracle):
    """8 x 12 x 12: one layer of 2 x 2 groups in a workgroup of six (hard threshold) or four (Wiener) wave pairs."""
    rng = np.random.default_rng(1)
    v = 300.0 + rng.normal(0, 6.0, (8, 12, 12))
    hit = rng.random(v.shape) < 0.05
    hit[:, :, :10] = False                       # bright voxels in the last two columns: the blocks at x = 4 stay alone
    v[hit] += rng.uniform(3000, 20000, int(hit.sum()))
    vol = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    f32 = vol.astype(np.float32)
    keys = oracle.blockmatch(f32, SIGMA, 3.0)
    assert keys.shape[:3] == (1, 2, 2) and group_sizes(keys) == {1, 8}
    _assert_stage(ctx, oracle, f32, keys)
    basic = oracle.bm4d(f32, SIGMA, stages=1)
    _assert_stage(ctx, oracle, f32, oracle.blockmatch(basic, SIGMA, 0.6), basic=basic)
    assert np.array_equal(_u16_gpu(ctx, vol, SIGMA, OFFSET), oracle.bm4d_u16(vol, SIGMA, OFFSET))


def test_batch_of_two_volumes_with_different_units(ctx, oracle, every_size):
    """The fp32 entry gives every volume of a batch its own numerator unit 2^(E - 43): the same volume at 1 x and
    at 1/64 x (sigma fixed) has E six apart and other group sizes."""
    f32 = every_size[1]
    vols = np.stack([f32, f32 / 64.0])
    got = ctx.denoise_f32_host(vols, SIGMA)
    for i in range(2):
        assert np.array_equal(got[i], oracle.bm4d(vols[i], SIGMA)), f"volume {i}"
