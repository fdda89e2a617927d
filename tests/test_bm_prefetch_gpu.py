"""The integer block-matching kernel's plane prefetch (bm_kernels.hip, bm_tile16_kernel): candidate planes are
staged by LDS-DMA one step ahead, the window rows are read by inline asm behind hand-placed waits and the cell's
own plane is loaded a step ahead of its use.  A missing or misplaced wait shows as a stale buffer (the plane of
the step before) or an early one, on some waves of some launches -- so the inputs must make a wrong plane visible:
the tables are (mostly) full, and they change when the volume is shifted by one plane.  Both conditions are
asserted on the CPU oracle before anything is compared; the tables must then equal the oracle's bit for bit,
launch after launch, with the carry between tiles off and forced.

Inputs (util.synth_volume, uint16; chosen on the CPU oracle alone):
  (40, 44, 64)   seed 2            y / x edge tiles and the clamped DMA rows   (seed 40 + 44 + 64 = 148 has only
                                   89.7 % of its tables full at c_match 3.0, sigma 24: below the condition)
  (72, 36, 68)   seed 176          three tiles per column, idle waves in the last one
  2 x 64^3       seeds 70, 71      the 4 x 16 tile shape, a batch
Bounds: c_match 3.0 at sigma 24, and c_match 0.6 at sigma 64 -- at sigma 24 the bound 0.6 admits next to nothing
on data of noise 24 and such a case would prove nothing; sigma 64 puts 0.6 above the 3.0 / 24 bound
(0.6 * 64^2 > 3.0 * 24^2), and on the oracle the tables are then 93 - 98 % full and 98 - 100 % of the blocks
change under the shift."""
import numpy as np
import pytest

from util import ctx_options, match_tables, synth_volume

from aind_exaspim_image_compression import _native

pytestmark = pytest.mark.gpu

CASES = {
    "edges_40x44x64": ((40, 44, 64), (2,)),
    "three_tiles_72x36x68": ((72, 36, 68), (176,)),
    "two_patches_64": ((64, 64, 64), (70, 71)),
}
BOUNDS = {"c3.0_sigma24": (24.0, 3.0), "c0.6_sigma64": (64.0, 0.6)}
_cache = {}


def _reference(oracle, case, bound):
    """(volumes [batch, nz, ny, nx] uint16, the oracle's tables [batch, gz, gy, gx, 16]); computed once, and the
    conditions on the inputs with them."""
    if (case, bound) not in _cache:
        shape, seeds = CASES[case]
        sigma, c_match = BOUNDS[bound]
        vols = np.stack([synth_volume(shape, seed=s, as_u16=True)[0] for s in seeds])
        want, full, changed = [], [], []
        for v in vols:
            f = v.astype(np.float32)               # blockmatch_u16 matches on the counts themselves
            k = oracle.blockmatch(f, sigma, c_match)
            shifted = oracle.blockmatch(np.roll(f, -1, 0), sigma, c_match)
            want.append(k)
            full.append(np.mean(k[..., 15] != _native.KEY_EMPTY))
            changed.append(np.mean(np.any(k != shifted, axis=-1)))
        print(f"{case} {bound}: tables full {np.round(full, 3)}, blocks that change under a one-plane shift "
              f"{np.round(changed, 3)}")
        assert min(full) >= 0.90, f"only {min(full):.3f} of the oracle's tables are full"
        assert min(changed) >= 0.90, f"only {min(changed):.3f} of the reference blocks change under the shift"
        want = np.stack(want)
        want.setflags(write=False)
        _cache[(case, bound)] = (vols, want)
    return _cache[(case, bound)]


@pytest.fixture
def carry(ctx):
    with ctx_options(ctx) as set_options:
        yield lambda n: set_options(bm_carry=n)      # 0 off, 1 automatic (large launches), 2 forced


@pytest.mark.parametrize("carry_mode", [0, 2], ids=["carry_off", "carry_forced"])
@pytest.mark.parametrize("bound", list(BOUNDS))
@pytest.mark.parametrize("case", list(CASES))
def test_tables_equal_the_oracle_launch_after_launch(ctx, oracle, carry, case, bound, carry_mode):
    vols, want = _reference(oracle, case, bound)
    sigma, c_match = BOUNDS[bound]
    carry(carry_mode)
    if carry_mode == 2:
        assert _native.blockmatch_plan(vols.shape[1:], batch=vols.shape[0], ctx=ctx)["carry"]
    for rep in range(3):       # the plane buffers and the carry slots are reused by every step, tile and launch
        np.testing.assert_array_equal(match_tables(ctx, vols, sigma, c_match), want, err_msg=f"launch {rep}")


def test_pipeline_equals_the_oracle(ctx, oracle):
    """Both block-matching launches inside the uint16 pipeline (the second one on the rounded basic estimate)."""
    shape, (seed,) = CASES["three_tiles_72x36x68"]
    vol = synth_volume(shape, seed=seed, as_u16=True)[0]
    want = oracle.bm4d_u16(vol, 24.0, 37.0)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    try:
        ctx.denoise_u16(d_in, d_out, shape, 24.0, 37.0)
        ctx.sync()
        got = d_out.download(shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()
    np.testing.assert_array_equal(got, want)
