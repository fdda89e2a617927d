"""The integer block-matching kernel walks its 88 steps as a loop over dz with, inside it, the four steps of the
six-row pass (dy <= 0), that pass's exchange and selection, the four steps of the five-row pass (dy > 0) and its
exchange and selection (bm_kernels.hip, bm_tile16_kernel).  A pass that is skipped, doubled, read
from the wrong plane buffer or selected with another pass's dy changes the candidates of its (dz, pass) class --
so every one of the 22 classes must supply entries to the tables under test.  That is asserted on the CPU oracle's
tables before anything is compared: the code of a key is 1 + ((dz + 5) * 11 + (dy + 5)) * 11 + dx + 5 (0: the
reference block itself, not counted), and each class has at least 50 entries per case.  The tables must then
equal the oracle's bit for bit, launched twice, with the carry between tiles off and forced.

Inputs (util.synth_volume, uint16) and bounds as in test_bm_prefetch_gpu.py:
  (40, 44, 64)   seed 2            y / x edge tiles
  (72, 36, 68)   seed 176          three tiles per column, idle waves in the last one
  2 x 64^3       seeds 70, 71      the 4 x 16 tile shape, a batch
  c_match 3.0 at sigma 24, and c_match 0.6 at sigma 64
"""
import numpy as np
import pytest

from util import ctx_options, match_tables, synth_volume

from aind_exaspim_image_compression import _native

CASES = {
    "edges_40x44x64": ((40, 44, 64), (2,)),
    "three_tiles_72x36x68": ((72, 36, 68), (176,)),
    "two_patches_64": ((64, 64, 64), (70, 71)),
}
BOUNDS = {"c3.0_sigma24": (24.0, 3.0), "c0.6_sigma64": (64.0, 0.6)}
MIN_PER_CLASS = 50
_cache = {}


def class_counts(keys):
    """Entries per (dz, pass) class, [11, 2]: pass 0 is dy <= 0, pass 1 is dy > 0."""
    k = keys[keys != _native.KEY_EMPTY]
    code = (k & 0x7FF).astype(np.int64)
    code = code[code > 0] - 1
    dz, dy = code // 121 - 5, (code // 11) % 11 - 5
    assert dz.min() >= -5 and dz.max() <= 5
    counts = np.zeros((11, 2), np.int64)
    np.add.at(counts, (dz + 5, (dy > 0).astype(np.int64)), 1)
    return counts


def _reference(oracle, case, bound):
    """(volumes [batch, nz, ny, nx] uint16, the oracle's tables [batch, gz, gy, gx, 16]); computed once, and the
    condition on the tables with them."""
    if (case, bound) not in _cache:
        shape, seeds = CASES[case]
        sigma, c_match = BOUNDS[bound]
        vols = np.stack([synth_volume(shape, seed=s, as_u16=True)[0] for s in seeds])
        want = np.stack([oracle.blockmatch(v.astype(np.float32), sigma, c_match) for v in vols])
        counts = class_counts(want)
        print(f"{case} {bound}: entries per (dz, pass) class, dy <= 0 {counts[:, 0].tolist()}, "
              f"dy > 0 {counts[:, 1].tolist()}")
        assert counts.min() >= MIN_PER_CLASS, f"a (dz, pass) class has only {counts.min()} entries: {counts.tolist()}"
        want.setflags(write=False)
        _cache[(case, bound)] = (vols, want)
    return _cache[(case, bound)]


@pytest.mark.parametrize("bound", list(BOUNDS))
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_tables_draw_on_every_dz_and_pass(oracle, case, bound):
    _reference(oracle, case, bound)


@pytest.fixture
def carry(ctx):
    with ctx_options(ctx) as set_options:
        yield lambda n: set_options(bm_carry=n)      # 0 off, 1 automatic (large launches), 2 forced


@pytest.mark.gpu
@pytest.mark.parametrize("carry_mode", [0, 2], ids=["carry_off", "carry_forced"])
@pytest.mark.parametrize("bound", list(BOUNDS))
@pytest.mark.parametrize("case", list(CASES))
def test_tables_equal_the_oracle_twice(ctx, oracle, carry, case, bound, carry_mode):
    vols, want = _reference(oracle, case, bound)
    sigma, c_match = BOUNDS[bound]
    carry(carry_mode)
    if carry_mode == 2:
        assert _native.blockmatch_plan(vols.shape[1:], batch=vols.shape[0], ctx=ctx)["carry"]
    for rep in range(2):
        got = match_tables(ctx, vols, sigma, c_match)
        if not np.array_equal(got, want):
            diff = class_counts(got) - class_counts(want)
            np.testing.assert_array_equal(got, want, err_msg=f"launch {rep}; entries per (dz, pass) class, got - "
                                                             f"oracle: {diff.tolist()}")
