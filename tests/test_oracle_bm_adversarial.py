"""The C oracle against the numpy restatement of the specification (tests/bm4d_pyref.py) on the inputs of
tests/bm_adversarial_inputs.py -- ties, keys on the admission bound, saturating cells, distances at the 2^24
gate -- and the conditions that make those inputs what they claim to be.  The second kind asserts properties of
the INPUTS (read off the oracle's tables), so that a change of a family cannot quietly take it off its edge.
CPU only; tests/test_bm_adversarial_gpu.py runs the kernels on the same inputs."""
import numpy as np
import pytest

import bm4d_pyref
import bm_adversarial_inputs as adv

SHAPE = (12, 13, 16)
EMPTY = np.uint32(0xFFFFFFFF)
_tables = {}


def _oracle_tables(oracle, name, sigma, c_match):
    key = (name, sigma, c_match)
    if key not in _tables:
        t = oracle.blockmatch(adv.volume(name, SHAPE).astype(np.float32), sigma, c_match)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def _distance_bits(keys):
    return keys & np.uint32(0xFFFFF800)


def _tied_neighbours(keys):
    """adjacent table entries with one quantised distance (the order between them is the displacement code's)"""
    valid = (keys[..., 1:] != EMPTY) & (keys[..., :-1] != EMPTY)
    return int(((_distance_bits(keys[..., 1:]) == _distance_bits(keys[..., :-1])) & valid).sum())


@pytest.mark.parametrize("name,sigma,c_match", [(n, s, c) for n, _, sig in adv.CASES for s, c in sig])
def test_oracle_tables_are_the_specifications(oracle, name, sigma, c_match):
    vol = adv.volume(name, SHAPE)
    assert vol.dtype == np.uint16 and vol.shape == SHAPE
    want = bm4d_pyref.blockmatch(vol.astype(np.float32), sigma, c_match)
    got = _oracle_tables(oracle, name, sigma, c_match)
    np.testing.assert_array_equal(got, want)
    assert oracle.keymax(sigma, c_match) == bm4d_pyref.keymax(sigma, c_match)


def test_inputs_are_deterministic():
    for name, make, _ in adv.CASES:
        np.testing.assert_array_equal(make(SHAPE), make(SHAPE), err_msg=name)
    assert (adv.ramp_perturbed(SHAPE).astype(np.int64) - adv.ramp(SHAPE)).min() == -1
    assert (adv.ramp_perturbed(SHAPE).astype(np.int64) - adv.ramp(SHAPE)).max() == 1


def test_full_range_checker_ties_every_admitted_candidate_at_zero(oracle):
    """Period 1, levels 0 / 65535: an even displacement maps the pattern onto itself, an odd one differs by 65535
    in every voxel -- full tables of distance 0, even displacements only."""
    keys = _oracle_tables(oracle, "checker-p1-0-65535", adv.SIGMA, 3.0)
    assert (keys != EMPTY).all()
    assert (_distance_bits(keys) == 0).all()
    assert (adv.displacement_sums(keys) % 2 == 0).all()


@pytest.mark.parametrize("lo,hi", adv.LEVELS)
def test_no_checker_admits_an_odd_displacement_at_period_one(oracle, lo, hi):
    """The worst candidates there are (every voxel differs by hi - lo); a cell sum that wraps or a difference that
    wraps instead of saturating would admit them, some at distance 0."""
    keys = _oracle_tables(oracle, f"checker-p1-{lo}-{hi}", adv.SIGMA, 3.0)
    assert (adv.displacement_sums(keys) % 2 == 0).all()
    assert (keys[..., 1] != EMPTY).all()                       # and the even ones are there


def test_the_level_pairs_sit_where_the_integer_kernel_could_break():
    d = [hi - lo for lo, hi in adv.LEVELS]
    assert d == [65535, 32767, 32768, 1 << 14, 1 << 13, 1 << 12]
    assert 64 * d[3] ** 2 == 1 << 34 and 64 * d[4] ** 2 == 1 << 32        # multiples of 2^32: a wrap reads 0
    assert 1 << 27 < 64 * d[5] ** 2 == 1 << 30 < 1 << 31                  # above the cap, below any wrap


def test_ramps_tie_at_non_zero_distance(oracle):
    """Measured on this shape: 189 to 191 adjacent ties on the ramp over the three sigmas, 24 to 25 on the
    perturbed one (the bounds, 100 and 10, ask for about half of that)."""
    for sigma, c_match in adv.BY_NAME["ramp"][1]:
        keys = _oracle_tables(oracle, "ramp", sigma, c_match)
        ties = keys[..., 1:][(_distance_bits(keys[..., 1:]) == _distance_bits(keys[..., :-1]))
                             & (keys[..., 1:] != EMPTY)]
        assert _tied_neighbours(keys) >= 100, (sigma, _tied_neighbours(keys))
        assert (_distance_bits(ties) != 0).any()
        assert _tied_neighbours(_oracle_tables(oracle, "ramp_perturbed", sigma, c_match)) >= 10, sigma


def test_ramp_sigmas_put_the_bound_on_a_distance_the_ramp_attains(oracle):
    """a distance in KEYMAX's bucket is admitted even when it exceeds c sigma^2 512.  With sigma =
    fl32(20 / sqrt 3) and fl32(28 / sqrt 3) the bound's bucket is that of S = 512 * 20^2 and 512 * 28^2, which the
    ramp attains (dx = +-1, dz = +-1): those entries are in the tables, and nothing beyond the bucket is."""
    for sigma, delta in ((adv.SIGMA_RAMP_X, 20), (adv.SIGMA_RAMP_Z, 28)):
        s_bits = int(np.float32(512.0 * delta * delta).view(np.uint32))
        assert s_bits & 0x7FF == 0
        assert oracle.keymax(sigma, 3.0) == s_bits + 0x800                  # KEYMAX ends exactly that bucket
        keys = _oracle_tables(oracle, "ramp", sigma, 3.0)
        valid = keys != EMPTY
        assert (_distance_bits(keys)[valid] <= s_bits).all()
        assert (_distance_bits(keys)[valid] == s_bits).any()               # in the last admitted bucket (tables
        #                                                                    that smaller distances fill hold none)


def test_loud_noise_fills_the_range_below_the_gate(oracle):
    assert 3.0 * adv.SIGMA_LOUD ** 2 * 512 < 1 << 24 < 3.0 * adv.SIGMA_LOUD_OVER ** 2 * 512
    assert 0.6 * adv.SIGMA_LOUD_WIENER ** 2 * 512 < 1 << 24
    keys = _oracle_tables(oracle, "loud_noise", adv.SIGMA_LOUD, 3.0)
    sizes = np.unique((keys != EMPTY).sum(axis=-1))
    assert sizes.min() == 1 and sizes.max() == 16 and sizes.size >= 5, sizes
    top = _distance_bits(keys[keys != EMPTY]).max()
    assert float(np.array([top], np.uint32).view(np.float32)[0]) > 0.95 * (1 << 24)


@pytest.mark.parametrize("v", [4.0, 5.0, 1000.0])
@pytest.mark.parametrize("lam", [2.0, 1.0])
def test_hard_threshold_keeps_a_coefficient_equal_to_the_threshold(oracle, v, lam):
    """DESIGN.md 3.6 zeroes |c| < lambda sigma: a coefficient EQUAL to the threshold stays.  A constant volume
    has one non-zero coefficient per group, the DC X; sigma = X / lambda and its fp32 neighbours decide."""
    sig = adv.hard_threshold_sigmas(oracle, v, lam)
    vol = np.full((13, 11, 10), v, dtype=np.float32)
    for s in sig[:2]:
        assert np.abs(oracle.bm4d(vol, s, stages=1, lambda_ht=lam) - vol).max() <= 1e-6 * v
    keys = oracle.blockmatch(vol, sig[2], 3.0)
    num, den = oracle.stage(vol, keys, sig[2], lambda_ht=lam)
    assert (num == 0).all() and (den > 0).all()                            # max(N, 1): a weight, no estimate
    assert (oracle.bm4d(vol, sig[2], stages=1, lambda_ht=lam) == 0).all()
