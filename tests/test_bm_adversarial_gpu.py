"""Block matching and the stage kernels on the inputs of tests/bm_adversarial_inputs.py -- exact ties at zero and
non-zero distance, keys in KEYMAX's bucket, cells whose every voxel saturates the int16 difference or whose sum is
a multiple of 2^32, distances up to the 2^24 gate, a coefficient equal to the hard threshold -- against the C oracle,
bit for bit.  tests/test_oracle_bm_adversarial.py holds the oracle to the specification's restatement on the same
inputs and asserts that they reach these edges; `synth_volume`, which every other BM4D test uses, reaches none."""
import numpy as np
import pytest

import bm_adversarial_inputs as adv
from util import ctx_options

from aind_exaspim_image_compression import _native

pytestmark = pytest.mark.gpu

# both tile shapes, ragged grids, the odd-nx fall-back of the integer kernel (test_integer_block_matching_equals_the_oracle)
SHAPES = [(24, 28, 32), (26, 31, 22), (24, 24, 25)]
TALL = (64, 64, 64)                              # the 4 x 16 tile shape; two tiles per column with the carry
TALL_FAMILIES = ("checker-p2-1000-17384", "ramp_perturbed", "loud_noise")
_want = {}


def _oracle_tables(oracle, name, shape, sigma, c_match):
    """The reference of one (input, bound), computed once and shared read-only by every path."""
    key = (name, shape, sigma, c_match)
    if key not in _want:
        t = oracle.blockmatch(adv.volume(name, shape).astype(np.float32), sigma, c_match)
        t.setflags(write=False)
        _want[key] = t
    return _want[key]


def _grid(shape):
    return tuple(len(_native.grid_positions(n)) for n in shape)


class _Matcher:
    """One or more volumes of a shape on the device, as fp32 and as uint16, and a table buffer."""

    def __init__(self, ctx, vols):
        self.ctx, self.shape, self.batch = ctx, vols[0].shape, len(vols)
        both = np.stack(vols)
        self.d_f32 = ctx.to_device(both.astype(np.float32))
        self.d_u16 = ctx.to_device(both)
        self.g = _grid(self.shape)
        self.d_keys = ctx.alloc(self.batch * int(np.prod(self.g)) * 16 * 4)

    def tables(self, u16, sigma, c_match, **options):
        ctx = self.ctx
        with ctx_options(ctx, **options):
            self.d_keys.fill(0x5A)
            call, vol = (ctx.blockmatch_u16, self.d_u16) if u16 else (ctx.blockmatch, self.d_f32)
            call(vol, self.shape, sigma, c_match, self.d_keys, batch=self.batch)
            ctx.sync()
            return self.d_keys.download((self.batch, *self.g, 16), np.uint32)

    def free(self):
        for b in (self.d_f32, self.d_u16, self.d_keys):
            b.free()


# (name of the path, uint16 entry point?, options)
PATHS = [("blockmatch", False, {}),
         ("blockmatch on a guarded copy", False, {"bm_guarded_copy": 1}),
         ("blockmatch, one-wave kernel", False, {"force_generic_bm": 1}),
         ("blockmatch_u16, integer kernel", True, {"bm_int": 1}),
         ("blockmatch_u16, float kernel", True, {"bm_int": 0})]
CARRY_PATHS = [("blockmatch with the carry", False, {"bm_carry": 2}),
               ("blockmatch_u16 with the carry", True, {"bm_carry": 2})]


@pytest.mark.parametrize("name", [n for n, _, _ in adv.CASES])
@pytest.mark.parametrize("shape", SHAPES)
def test_match_tables_equal_the_oracle_on_every_path(ctx, oracle, shape, name):
    m = _Matcher(ctx, [adv.volume(name, shape)])
    try:
        for sigma, c_match in adv.BY_NAME[name][1]:
            want = _oracle_tables(oracle, name, shape, sigma, c_match)
            for what, u16, options in PATHS:
                got = m.tables(u16, sigma, c_match, **options)[0]
                np.testing.assert_array_equal(got, want, err_msg=f"{what}: {name} {shape} sigma {sigma} c {c_match}")
    finally:
        m.free()


@pytest.mark.parametrize("name", TALL_FAMILIES)
def test_match_tables_of_a_patch_with_and_without_the_carry(ctx, oracle, name):
    m = _Matcher(ctx, [adv.volume(name, TALL)])
    try:
        assert not _native.blockmatch_plan(TALL, ctx=ctx)["carry"]            # a small launch: off unless forced
        with ctx_options(ctx, bm_carry=2):
            assert _native.blockmatch_plan(TALL, ctx=ctx)["carry"]
        for sigma, c_match in adv.BY_NAME[name][1]:
            want = _oracle_tables(oracle, name, TALL, sigma, c_match)
            for what, u16, options in PATHS + CARRY_PATHS:
                got = m.tables(u16, sigma, c_match, **options)[0]
                np.testing.assert_array_equal(got, want, err_msg=f"{what}: {name} sigma {sigma} c {c_match}")
    finally:
        m.free()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_batch_of_two_families(ctx, oracle, shape):
    """One launch over a wrapping checkerboard and the ramp: each element gets its own tables."""
    names = ("checker-p1-1000-9192", "ramp")
    m = _Matcher(ctx, [adv.volume(n, shape) for n in names])
    try:
        for u16 in (False, True):
            got = m.tables(u16, adv.SIGMA, 3.0)
            for i, n in enumerate(names):
                np.testing.assert_array_equal(got[i], _oracle_tables(oracle, n, shape, adv.SIGMA, 3.0),
                                              err_msg=f"element {i} ({n}), uint16 entry {u16}")
    finally:
        m.free()


PIPELINE_INPUTS = [(f"checker-p{p}-{lo}-{hi}", adv.SIGMA) for p in (1, 2) for lo, hi in adv.LEVELS] + \
                  [("loud_noise", adv.SIGMA_LOUD), ("ramp_perturbed", adv.SIGMA)]


@pytest.mark.parametrize("name,sigma", PIPELINE_INPUTS)
@pytest.mark.parametrize("shape", [(24, 28, 32), (26, 31, 22)])
def test_uint16_pipeline_on_data_that_fills_the_fixed_point_range(ctx, oracle, shape, name, sigma):
    """Both stages of exabm4d_denoise_u16_dev: stage 2's integer matching on the rounded basic estimate, both
    stage kernels on groups whose coefficients reach 90 * 65535, and the final clamp."""
    vol = adv.volume(name, shape)
    d_in, d_out = ctx.to_device(vol), ctx.alloc(vol.nbytes)
    try:
        for offset in (37.0, 0.0):
            want = oracle.bm4d_u16(vol, sigma, offset)
            d_out.fill(0xEE)
            ctx.denoise_u16(d_in, d_out, shape, sigma, offset)
            ctx.sync()
            np.testing.assert_array_equal(d_out.download(shape, np.uint16), want, err_msg=f"offset {offset}")
    finally:
        d_in.free()
        d_out.free()


def _stage(ctx, vol, keys, sigma, params):
    bufs = [ctx.to_device(vol), ctx.to_device(keys), ctx.alloc(vol.nbytes).fill(0xFF), ctx.alloc(vol.nbytes).fill(0xFF)]
    try:
        ctx.stage(bufs[0], None, bufs[1], vol.shape, sigma, bufs[2], bufs[3], params=params)
        ctx.sync()
        return bufs[2].download(vol.shape, np.float32), bufs[3].download(vol.shape, np.float32)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("v", [4.0, 5.0, 1000.0])
@pytest.mark.parametrize("lam", [2.0, 1.0])
def test_hard_threshold_keeps_a_coefficient_equal_to_the_threshold(ctx, oracle, lam, v):
    """DESIGN.md 3.6 zeroes |c| < lambda sigma.  A constant volume has one non-zero coefficient per group, the DC
    X; with sigma_eq = fl32(X / lambda) the threshold IS X.  At sigma_eq and the fp32 number below it the
    coefficient stays (the volume comes back), at the number above it the whole group is shrunk: estimate 0, weight
    1 / max(N, 1) > 0.  `<` against `<=` in a kernel shows here and nowhere else in the suite."""
    params = _native.default_params(lambda_ht=lam)
    sigmas = adv.hard_threshold_sigmas(oracle, v, lam)
    for shape in ((16, 16, 20), (13, 11, 10)):
        vol = np.full(shape, v, dtype=np.float32)
        for i, sigma in enumerate(sigmas):
            what = f"{shape} sigma {sigma!r} ({('below', 'at', 'above')[i]} X / lambda)"
            got = ctx.denoise_f32_host(vol, sigma, params=params, stages=1)
            np.testing.assert_array_equal(got, oracle.bm4d(vol, sigma, stages=1, lambda_ht=lam), err_msg=what)
            keys = oracle.blockmatch(vol, sigma, 3.0)
            assert (keys != 0xFFFFFFFF).all()                                  # groups of 16, as X assumes
            num_w, den_w = oracle.stage(vol, keys, sigma, lambda_ht=lam)
            num_g, den_g = _stage(ctx, vol, keys, sigma, params)
            np.testing.assert_array_equal(den_g, den_w, err_msg=what)
            np.testing.assert_array_equal(num_g, num_w, err_msg=what)
            assert (den_g > 0).all()
            if i < 2:                                                          # the specification's reading
                assert np.abs(got - vol).max() <= 1e-6 * v, what
            else:
                assert (got == 0).all() and (num_g == 0).all(), what
