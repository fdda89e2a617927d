"""Inputs that put block matching and the stages on their edges (numpy only, deterministic): exact ties,
admission keys on and next to KEYMAX, differences that saturate int16 in every voxel of a cell, cell sums
at and beyond the integer kernel's cap and the int32 range, distances up to the 2^24 gate between the integer
and the float kernel.  `synth_volume` reaches none of these.  Every volume is uint16, so the fp32 entry points
(on `v.astype(float32)`) and the uint16 ones see the same counts.

`CASES` lists every family with the (sigma, c_match) pairs that go with it; tests/test_oracle_bm_adversarial.py
asserts, on the oracle's tables, that each input reaches the edge it was built for."""
import numpy as np

PERIODS = (1, 2, 4)
# int16 subtraction is exact up to 32767 and saturates from 32768; differences of 2^13 and 2^14 make a cell's
# sum of squares 64 * 2^26 = 2^32 and 64 * 2^28 = 2^34 (a wrapping accumulator reads 0: the best match instead
# of the worst); 2^12 gives 2^30, beyond bm_tile16_kernel's 2^27 cap and below any wrap
LEVELS = ((0, 65535), (0, 32767), (0, 32768), (1000, 1000 + 16384), (1000, 1000 + 8192), (1000, 1000 + 4096))


def fl32(x):
    return float(np.float32(x))


SIGMA = 24.0
SIGMA_RAMP_X = fl32(20.0 / np.sqrt(3.0))     # 3 sigma^2 512 ~ 512 * 20^2: KEYMAX ends the key bucket of S = 204800
SIGMA_RAMP_Z = fl32(28.0 / np.sqrt(3.0))     # ... of 512 * 28^2
SIGMA_LOUD = 104.5                           # 3 * 104.5^2 * 512 = 16 773 504 < 2^24: the integer kernel runs
SIGMA_LOUD_OVER = 104.52                     # ... 16 779 925 > 2^24: the float kernel has to
SIGMA_LOUD_WIENER = 233.6                    # 0.6 * 233.6^2 * 512 = 16 763 781: stage 2's factor below the gate
LOUD_SEED = 3          # on 12 x 13 x 16: table sizes 1 ... 16, largest admitted S = 0.9988 * 2^24 (seeds 0-2, 4, 5 miss one)


def _grid(shape):
    return np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")


def checker(shape, period, lo, hi):
    """`lo` where (z // p + y // p + x // p) is even, else `hi`."""
    z, y, x = _grid(shape)
    odd = ((z // period + y // period + x // period) & 1).astype(bool)
    return np.where(odd, hi, lo).astype(np.uint16)


def ramp(shape):
    """1000 + 20 x + 24 y + 28 z: a displacement d differs by the constant 20 dx + 24 dy + 28 dz in every voxel,
    S = 512 delta^2 exactly, and many displacements share a delta -- exact ties at non-zero distance."""
    z, y, x = _grid(shape)
    v = 1000 + 20 * x + 24 * y + 28 * z
    assert v.max() <= 65535
    return v.astype(np.uint16)


def ramp_perturbed(shape, seed=7):
    """The ramp with +-1 count on about 2 % of the voxels: S moves by a few tens, inside and just across one
    2^-12 key quantum."""
    rng = np.random.default_rng(seed)
    v = ramp(shape).astype(np.int64)
    hit = rng.random(shape) < 0.02
    v[hit] += rng.choice([-1, 1], size=int(hit.sum()))
    return v.astype(np.uint16)


def step_edge(shape):
    """Level 100, level 107 from x = 9 on: distances are multiples of 64 * 49."""
    v = np.full(shape, 100, dtype=np.uint16)
    v[:, :, 9:] = 107
    return v


def loud_noise(shape, seed=LOUD_SEED):
    """rint(N(2000, 140)): with sigma 104.5 tables hold 1 to 16 entries and admitted distances reach the 2^24 gate."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(2000.0, 140.0, shape)), 0, 65535).astype(np.uint16)


def _cases():
    out = []
    for p in PERIODS:
        for lo, hi in LEVELS:
            out.append((f"checker-p{p}-{lo}-{hi}", (lambda s, p=p, lo=lo, hi=hi: checker(s, p, lo, hi)),
                        ((SIGMA, 3.0),)))
    on_ramp = ((SIGMA, 3.0), (SIGMA_RAMP_X, 3.0), (SIGMA_RAMP_Z, 3.0))
    out.append(("ramp", ramp, on_ramp))
    out.append(("ramp_perturbed", ramp_perturbed, on_ramp))
    out.append(("step_edge", step_edge, ((SIGMA, 3.0),)))
    out.append(("loud_noise", loud_noise, ((SIGMA, 3.0), (SIGMA_LOUD, 3.0), (SIGMA_LOUD_OVER, 3.0),
                                           (SIGMA_LOUD_WIENER, 0.6))))
    return out


CASES = _cases()                                     # (name, shape -> uint16 volume, ((sigma, c_match), ...))
BY_NAME = {name: (make, sigmas) for name, make, sigmas in CASES}


def volume(name, shape):
    return BY_NAME[name][0](shape)


def displacement_sums(keys):
    """dz + dy + dx of every entry of a match table array (0 for the block itself and for unused slots)."""
    code = (keys & np.uint32(0x7FF)).astype(np.int64)
    c = np.maximum(code - 1, 0)
    s = (c // 121 - 5) + ((c // 11) % 11 - 5) + (c % 11 - 5)
    return np.where((code == 0) | (keys == np.uint32(0xFFFFFFFF)), 0, s)


def hard_threshold_sigmas(oracle, v, lam):
    """(sigma_dn, sigma_eq, sigma_up): lambda * sigma_eq is the DC of a group of 16 constant blocks, exactly."""
    G = oracle.group_transform(np.full((16, 8, 8, 8), v, dtype=np.float32))
    X = np.float32(G[0, 0, 0, 0])
    rest = G.copy()
    rest[0, 0, 0, 0] = 0
    assert X > 0 and (rest == 0).all()
    eq = np.float32(X / np.float32(lam))
    assert np.float32(np.float64(np.float32(lam)) * np.float64(eq)) == X        # 3.6's product: the threshold is X
    dn, up = np.nextafter(eq, np.float32(0)), np.nextafter(eq, np.float32(np.inf))
    return float(dn), float(eq), float(up)
