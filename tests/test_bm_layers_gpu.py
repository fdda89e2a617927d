"""Integer block matching with 8 and with 12 cell layers per tile (option `bm_layers`).

The 12-layer tile runs twelve waves per workgroup and exchanges a pass's cell sums in rounds of two dy rows
(2 + 2 + 2 and 2 + 2 + 1) where the 8-layer tile takes rounds of three (3 + 3 and 3 + 2); the carry slot of a
(dz, pass) is linear in the dy row, so both geometries read and write it at `row * 11 * 64`.  Every case forces
both geometries, with the carry between the tiles of a column off and forced on, and asserts that the match
tables equal the oracle's bit for bit.  The z extents are the ones at which the new geometry can go wrong: a
tile with idle waves (the barrier count), a full tile, a second tile of ONE working wave whose lower layer is
carried, three tiles, and two tile rows in y (two carry columns, staged rows clamping at both y edges).
Nothing here provokes an error path."""
import numpy as np
import pytest

import bm_adversarial_inputs as adv

pytestmark = pytest.mark.gpu

SIGMA = 24.0
PEDESTAL = 37.0
BOUNDS = ((SIGMA, 3.0), (SIGMA, 0.6))            # (sigma, c_match) of the hard-threshold and the Wiener stage
GEOMETRIES = [(layers, carry) for layers in (8, 12) for carry in (0, 2)]
# (z, y, x) of the uint16 volume; z / 4 cell layers
SHAPES = [(40, 36, 36),      # 10 layers: one 12-layer tile with two idle waves
          (48, 36, 36),      # 12 layers: one full tile, nothing carried
          (52, 36, 40),      # 13 layers: the second tile has one working wave, its lower layer carried
          (100, 36, 36),     # 25 layers: three tiles, the last one with a single wave
          (104, 64, 36)]     # 26 layers, two tile rows in y
ADV_SHAPE = (52, 36, 40)


@pytest.fixture
def geometry(ctx):
    """Sets (bm_layers, bm_carry); both are back at the library's defaults afterwards."""
    def set_geometry(layers, carry):
        ctx.set_option("bm_layers", layers)
        ctx.set_option("bm_carry", carry)
    try:
        yield set_geometry
    finally:
        ctx.set_option("bm_layers", 0)
        ctx.set_option("bm_carry", 1)


def _noise(shape):
    rng = np.random.default_rng(sum(shape))
    return np.clip(np.rint(rng.normal(PEDESTAL, SIGMA, shape)), 0, 65535).astype(np.uint16)


def _dy_of(keys):
    """dy of every table entry (-99 for the block itself and for unused slots)."""
    code = (keys & np.uint32(0x7FF)).astype(np.int64)
    dy = ((code - 1) // 11) % 11 - 5
    return np.where((code == 0) | (keys == np.uint32(0xFFFFFFFF)), -99, dy)


def _tables_in_every_geometry(ctx, geometry, vol, sigma, c_match):
    from aind_exaspim_image_compression import _native
    g = [len(_native.grid_positions(n)) for n in vol.shape]
    d_vol = ctx.to_device(vol)
    d_keys = ctx.alloc(g[0] * g[1] * g[2] * 16 * 4)
    got = {}
    try:
        for layers, carry in GEOMETRIES:
            geometry(layers, carry)
            ctx.blockmatch_u16(d_vol, vol.shape, sigma, c_match, d_keys)
            ctx.sync()
            got[layers, carry] = d_keys.download((*g, 16), np.uint32)
    finally:
        d_vol.free()
        d_keys.free()
    return got


def _assert_every_geometry_gives_the_oracles_tables(ctx, oracle, geometry, vol, sigma, c_match, want=None):
    if want is None:
        want = oracle.blockmatch(vol.astype(np.float32) - np.float32(PEDESTAL), sigma, c_match)
    got = _tables_in_every_geometry(ctx, geometry, vol, sigma, c_match)
    for (layers, carry), keys in got.items():
        np.testing.assert_array_equal(keys, want, err_msg=f"bm_layers {layers}, bm_carry {carry}: against the oracle")
    for (layers, carry), keys in got.items():
        np.testing.assert_array_equal(keys, got[8, 0], err_msg=f"bm_layers {layers}, bm_carry {carry}: against 8 / 0")


def test_option_takes_0_8_and_12_only(ctx, geometry):
    for value in (8, 12, 0):
        ctx.set_option("bm_layers", value)
    for value in (-1, 6, 7, 16):
        with pytest.raises(ValueError, match="bm_layers"):         # EXABM4D_ERR_INVALID, as the binding raises it
            ctx.set_option("bm_layers", value)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_on_a_pedestal(ctx, oracle, geometry, shape):
    """Both stages' admission bounds.  Under the hard-threshold stage's bound nearly every candidate of pure noise
    is admitted, so the five-row pass's last round -- the single dy = 5 row of the 12-layer tile -- fills table
    entries: checked on the oracle's tables."""
    vol = _noise(shape)
    f = vol.astype(np.float32) - np.float32(PEDESTAL)
    for sigma, c_match in BOUNDS:
        want = oracle.blockmatch(f, sigma, c_match)
        if c_match == 3.0:
            assert (_dy_of(want) == 5).any(), "no table entry from dy = 5: the input misses the last round"
        _assert_every_geometry_gives_the_oracles_tables(ctx, oracle, geometry, vol, sigma, c_match, want)


@pytest.mark.parametrize("name", [name for name, _, _ in adv.CASES])
def test_adversarial_inputs(ctx, oracle, geometry, name):
    """Ties, keys in KEYMAX's bucket, saturating cells (tests/bm_adversarial_inputs.py) at 13 cell layers: the
    carried layer of the second tile holds them too."""
    vol = adv.volume(name, ADV_SHAPE)
    for sigma, c_match in adv.BY_NAME[name][1]:
        want = oracle.blockmatch(vol.astype(np.float32), sigma, c_match)
        _assert_every_geometry_gives_the_oracles_tables(ctx, oracle, geometry, vol, sigma, c_match, want)


def test_pipeline_u16_in_both_geometries(ctx, oracle, geometry):
    """exabm4d_denoise_u16_dev, two stages, on 26 cell layers: both matching launches in either geometry."""
    shape = (104, 40, 44)
    vol = _noise(shape)
    vol[30:70, 10:30, 12:34] += 300
    want = oracle.bm4d_u16(vol, SIGMA, PEDESTAL)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    got = {}
    try:
        for layers, carry in ((8, 1), (12, 1), (12, 2)):
            geometry(layers, carry)
            ctx.denoise_u16(d_in, d_out, shape, SIGMA, PEDESTAL)
            ctx.sync()
            got[layers, carry] = d_out.download(shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()
    for key, out in got.items():
        np.testing.assert_array_equal(out, want, err_msg=f"bm_layers, bm_carry = {key}: against the oracle")
        np.testing.assert_array_equal(out, got[8, 1], err_msg=f"bm_layers, bm_carry = {key}: against 8 layers")
