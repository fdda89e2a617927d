"""Seeded inputs of the validation-scoring tests and of their fixture (tests/golden/validate_batch.npz).

The fixture stores the reference's outputs only; tests/golden/make_validate_golden.py and the tests regenerate
every input from here.  numpy only, so the GPU machine regenerates them too.

A case is ``(pred, raw, target, fg_mask)``, each (B, z, y, x); COMBOS names the element types of pred / raw /
target.  SHAPES are the smallest at which the kernels take another path: fewer voxels than a workgroup has
threads with an odd and an even count (one / two middle elements), a count that is a multiple of no workgroup
size, several patches of a few waves, and the real 64^3 patch (several statistics workgroups per patch)."""
import numpy as np

U16, F32 = np.uint16, np.float32
COMBOS = {"val": (U16, F32, U16), "u16": (U16, U16, U16), "f32": (F32, F32, F32)}
SHAPES = [(2, (3, 5, 7)), (3, (5, 6, 7)), (1, (16, 16, 17)), (5, (16, 16, 16)), (2, (64, 64, 64))]
PCTS = (0.0, 0.1, 50.0)
SMALL = (5, 6, 7)       # content cases: 210 voxels, two middle elements


def _cast(a, dtype, offset=0.0):
    """Counts as uint16, or offset-subtracted counts as float32 (negative values included)."""
    if dtype == U16:
        return np.rint(a).clip(0, 65535).astype(U16)
    return (a - offset).astype(F32)


def random_batch(batch, shape, combo, seed):
    """Noise around 100 counts with sparse bright voxels; pred and target are two denoised versions of raw."""
    rng = np.random.default_rng(seed)
    full = (batch,) + tuple(shape)
    signal = 100.0 + 900.0 * (rng.random(full) < 0.03) * rng.random(full)
    raw = signal + rng.normal(0.0, 12.0, full)
    target = signal + rng.normal(0.0, 2.0, full)
    pred = signal + rng.normal(0.0, 3.0, full) + 40.0 * (rng.random(full) < 0.01)
    mask = (signal > 130.0) | (rng.random(full) < 0.02)
    tp, tr, tt = COMBOS[combo]
    return _cast(pred, tp, 100.37), _cast(raw, tr, 100.37), _cast(target, tt, 100.37), mask


def shape_cases():
    """name -> case: every shape with every dtype combination, random data."""
    cases = {}
    for i, (batch, shape) in enumerate(SHAPES):
        for j, combo in enumerate(COMBOS):
            cases[f"{combo}_{batch}x{'x'.join(map(str, shape))}"] = random_batch(batch, shape, combo, 100 + 10 * i + j)
    return cases


def content_cases():
    """name -> case: the data at which a selection or a reduction goes wrong, three patches of SMALL each."""
    cases = {}
    n = int(np.prod(SMALL))
    full = (3,) + SMALL

    pred, raw, target, mask = random_batch(3, SMALL, "val", 7)
    raw = np.stack([np.full(SMALL, 250.0, F32), np.full(SMALL, -3.625, F32), np.full(SMALL, 0.0, F32)])
    cases["constant_raw"] = (pred, raw, target, mask)                      # MAD is 0: only the + 1e-6 is left

    rng = np.random.default_rng(8)
    ties_raw = rng.integers(1000, 1004, full).astype(U16)
    ties_pred = rng.integers(1000, 1003, full).astype(U16)
    cases["ties_u16"] = (ties_pred, ties_raw, rng.integers(999, 1003, full).astype(U16), ties_raw > 1001)
    cases["ties_f32"] = (ties_pred.astype(F32) / 4, ties_raw.astype(F32) / 4 - 250.5, ties_pred.astype(F32) / 4,
                         ties_raw > 1001)

    pred, raw, target, mask = random_batch(3, SMALL, "f32", 9)
    cases["negative_raw"] = (pred, (raw - 4000.0).astype(F32), target, mask)

    pred, raw, target, mask = random_batch(3, SMALL, "val", 10)
    mask = mask.copy()
    mask[0], mask[1] = True, False                                          # all, none, mixed in one batch
    cases["mask_all_none_mixed"] = (pred, raw, target, mask)
    cases["mask_uint8"] = (pred, raw, target, mask.astype(np.uint8) * 7)    # non-zero is foreground
    cases["mask_float"] = (pred, raw, target, np.where(mask, 0.75, 0.5).astype(F32))    # > 0.5, strictly

    pred, raw, target, mask = random_batch(3, SMALL, "val", 11)
    raw = raw.copy()
    raw[1, 2, 3, 4] = np.nan
    raw[2, 0, 0, 0] = np.inf
    raw[2, 4, 5, 6] = -np.inf
    cases["nan_inf_raw"] = (pred, raw, target, mask)                        # patch 0 is clean

    pred, raw, target, mask = random_batch(3, SMALL, "f32", 12)
    pred = pred.copy()
    pred[0].reshape(-1)[-1] = np.nan
    cases["nan_pred"] = (pred, raw, target, mask)

    raw = raw.copy()
    raw[1].reshape(-1)[:n // 2 + 1] = np.inf                                # an infinite median: |inf - inf|
    cases["inf_median"] = (pred[::-1].copy(), raw, target, mask)

    # the two middle values are neighbouring float32 numbers: their mean is no float32
    one, up = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    half = np.r_[rng.uniform(-5.0, 0.5, n // 2 - 1), one, up, rng.uniform(1.5, 9.0, n // 2 - 1)].astype(F32)
    raw = np.stack([rng.permutation(half).reshape(SMALL) for _ in range(3)])
    raw[2] *= F32(-1024.0)
    pred, _, target, mask = random_batch(3, SMALL, "f32", 13)
    cases["halfway_median"] = (pred, raw, target, mask)

    # uint16's ends, and a prediction whose maximum is below raw's: the reference's uint16 difference wraps
    pred, raw, target, mask = random_batch(3, SMALL, "u16", 14)
    raw, pred = raw.copy(), pred.copy()
    raw[0, 0, 0, :3] = (0, 65535, 65535)
    pred[1, 1, 1, :2] = (65535, 0)
    cases["u16_ends"] = (pred, raw, target, mask)
    return cases


def all_cases():
    cases = shape_cases()
    cases.update(content_cases())
    return cases


def validate_batches(seed=21):
    """Three 16^3 examples in two batches (2 + 1) for train.validate: ``(x, y, raw, fg_mask)`` per batch, x and y
    float32 (B, 1, z, y, x) in the transform domain of ``transform_args()``, raw float32 counts, fg_mask float."""
    rng = np.random.default_rng(seed)
    shape = (3, 1, 16, 16, 16)
    off, scale, maxc = transform_args()
    signal = 120.0 + 800.0 * (rng.random(shape) < 0.04) * rng.random(shape)
    raw = (signal + rng.normal(0.0, 10.0, shape)).astype(F32)
    norm = np.arcsinh((maxc - off) / scale)
    x = (np.arcsinh((signal + rng.normal(0.0, 3.0, shape) - off) / scale) / norm).astype(F32)
    y = (np.arcsinh((signal + rng.normal(0.0, 1.0, shape) - off) / scale) / norm).astype(F32)
    mask = (signal > 150.0).astype(F32)
    return [(x[:2], y[:2], raw[:2], mask[:2]), (x[2:], y[2:], raw[2:], mask[2:])]


def transform_args():
    """AsinhTransform(offset, scale, max_count) of validate_batches."""
    return 90.0, 32.0, 65535.0


def inputs_digest():
    """sha256 over every regenerated input, in a fixed order (stored in the fixture)."""
    import hashlib
    h = hashlib.sha256()
    cases = all_cases()
    for name in cases:
        h.update(name.encode())
        for a in cases[name]:
            a = np.ascontiguousarray(a)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()
