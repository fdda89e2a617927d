"""The integer block-matching kernel's step addresses (bm_kernels.hip).  A lane keeps 32-bit byte
offsets for its LDS-DMA chunks and its cell's rows, one set per pass because staged rows clamp at the y edges, and
a step adds them to a plane base held in scalar registers.  Every sum, key and address is the one of before, so
the match tables of blockmatch_u16 must equal the oracle's orc_blockmatch exactly: tiles whose rows clamp low, not
at all, high, and on both sides at once; the first tile column (the base lies before the plane's row) and the last
(staged columns run past the row end); both tile shapes; with and without the carry."""
import numpy as np
import pytest

from util import ctx_options, match_tables

from aind_exaspim_image_compression import _native

pytestmark = pytest.mark.gpu
SIGMA = 24.0
C_MATCH = 3.0


def _volume(shape, seed):
    """Seeded noise on a ramp; a slab of voxels alternating 0 and 65535 (differences saturate the int16
    subtraction: such candidates must be rejected, never wrap); a constant region (all distances 0: ties, decided by
    the displacement code)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = 300.0 + 3.0 * zz + 2.0 * yy + 1.0 * xx + rng.normal(0.0, SIGMA, shape)
    vol = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    slab = vol[nz // 2:nz // 2 + 6, : ny // 2, nx // 4:]
    slab[...] = np.where((np.indices(slab.shape).sum(axis=0) & 1) == 1, 65535, 0).astype(np.uint16)
    vol[: nz // 3, ny - 14:, : nx // 2 + 3] = 1234
    return vol


def _keys(ctx, vols):
    return match_tables(ctx, vols, SIGMA, C_MATCH)


@pytest.fixture
def options(ctx):
    with ctx_options(ctx) as set_options:       # bm_carry: 0 off, 1 automatic, 2 forced
        yield lambda carry, xcd_mode=2: set_options(bm_carry=carry, bm_xcd_mode=xcd_mode)


@pytest.fixture(scope="module")
def three_rows(oracle):
    """72 x 72 x 40: 17 x 17 x 9 reference positions = three tiles in z (two carries), three tile rows (clamped low,
    interior, clamped high), two tile columns."""
    vol = _volume((72, 72, 40), 7)
    want = oracle.blockmatch(vol.astype(np.float32), SIGMA, C_MATCH)
    want.setflags(write=False)
    return vol, want


@pytest.mark.parametrize("carry", [2, 0])
def test_clamped_and_interior_tile_rows_both_edge_columns(ctx, options, three_rows, carry):
    vol, want = three_rows
    assert tuple(len(_native.grid_positions(n)) for n in vol.shape) == (17, 17, 9)
    options(carry)
    assert bool(_native.blockmatch_plan(vol.shape, ctx=ctx)["carry"]) == (carry == 2)
    np.testing.assert_array_equal(_keys(ctx, vol), want)


@pytest.mark.parametrize("xcd_mode", [0, 2])
def test_tile_orders_and_a_second_launch(ctx, options, three_rows, xcd_mode):
    """The slots of a column are written by every second tile and by every launch: the second launch finds the
    first one's carried layers in them."""
    vol, want = three_rows
    options(2, xcd_mode)
    first = _keys(ctx, vol)
    second = _keys(ctx, vol)
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(second, first)


def test_every_staged_row_clamped_on_both_sides(ctx, options, oracle):
    """24 rows for the 37 a plane stages: a single (y, x) tile whose staged rows leave the volume at both ends."""
    vol = _volume((40, 24, 32), 11)
    options(1)
    np.testing.assert_array_equal(_keys(ctx, vol), oracle.blockmatch(vol.astype(np.float32), SIGMA, C_MATCH))


def test_two_patches_in_the_flat_tile_shape(ctx, options, oracle):
    """64^3 patches take the 4 x 16 tiles (five tile rows, interior and edge ones; a 76-column window over a 64-voxel
    row), two tiles in z with the carry, both patches' columns in one slab."""
    vols = np.stack([_volume((64, 64, 64), 21), _volume((64, 64, 64), 22)])
    options(2)
    plan = _native.blockmatch_plan((64, 64, 64), ctx=ctx)
    assert plan["carry"]
    got = _keys(ctx, vols)
    for i in range(2):
        np.testing.assert_array_equal(got[i], oracle.blockmatch(vols[i].astype(np.float32), SIGMA, C_MATCH),
                                      err_msg=f"patch {i}")
