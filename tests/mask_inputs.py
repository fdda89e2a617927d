"""Seeded inputs of the mask / coherence-gate fixture (tests/golden/masks.npz).

The fixture stores outputs only; tests/golden/make_mask_golden.py and the tests regenerate every
input from here.  numpy only, so the GPU machine regenerates them too."""
import numpy as np

FG_SHAPE = (32, 32, 32)
ODD_SHAPE = (37, 64, 50)
GATE_SHAPE = (40, 40, 40)
LAGS = (1, 2, 3)


def _background(rng, shape, level=100.0, sd=4.0):
    return rng.normal(level, sd, shape)


def _tube(shape, axis=2, center=(12.0, 17.0), radius2=6.0, amp=600.0):
    """A bright, smooth tube along ``axis`` (a neurite stand-in, PSF-like falloff)."""
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    others = [g for a, g in enumerate(grids) if a != axis]
    r2 = (others[0] - center[0]) ** 2 + (others[1] - center[1]) ** 2
    return amp * np.exp(-r2 / radius2)


def smooth_blob(shape=GATE_SHAPE, lo=8, hi=32, amp=800.0, width=2.5):
    """A bright, spatially smooth block with soft edges: the coherent segment."""
    v = np.ones(shape, dtype=np.float64)
    for axis, s in enumerate(shape):
        x = np.arange(s, dtype=np.float64)
        prof = 1.0 / (1.0 + np.exp(-(x - lo) / width)) - 1.0 / (1.0 + np.exp(-(x - hi) / width))
        v = v * prof.reshape([-1 if a == axis else 1 for a in range(3)])
    return (amp * v).astype(np.float32)


def salt_pepper(shape=GATE_SHAPE, lo=8, hi=32, amp=900.0, rate=0.4, seed=0):
    """A bright, spatially incoherent salt-and-pepper block and its region: the artifact."""
    rng = np.random.default_rng(seed)
    region = np.zeros(shape, dtype=bool)
    region[lo:hi, lo:hi, lo:hi] = True
    v = np.zeros(shape, dtype=np.float32)
    v[(rng.random(shape) < rate) & region] = amp
    return v, region


def foreground_cases():
    """name -> (raw, k, dilate) for make_foreground_mask."""
    rng = np.random.default_rng(101)
    cases = {}
    u16 = np.rint(_background(rng, FG_SHAPE) + _tube(FG_SHAPE)).clip(0, 65535).astype(np.uint16)
    cases["u16_k6_d1"] = (u16, 6.0, 1)
    f32 = (_background(rng, FG_SHAPE, 100.0, 3.3) + _tube(FG_SHAPE, axis=0) - 100.37).astype(np.float32)
    cases["f32_offset_k6_d1"] = (f32, 6.0, 1)
    zero = np.zeros(FG_SHAPE, dtype=np.float32)        # MAD is 0: only the + 1e-6 is left
    zero[5, 6, 7] = 3.0
    zero[20:22, 3, 30] = 1e-5
    zero[31, 31, 31] = 2e-6
    cases["zero_block_k6_d1"] = (zero, 6.0, 1)
    odd = (_background(rng, ODD_SHAPE, 30.0, 5.0) + _tube(ODD_SHAPE, axis=1, center=(18.0, 25.0), amp=90.0)
           - 29.5).astype(np.float32)
    for k in (3.0, 6.0):
        for dilate in (0, 1, 2, 3):
            cases[f"odd_k{int(k)}_d{dilate}"] = (odd, k, dilate)
    even_small = np.rint(_background(rng, (6, 5, 4), 50.0, 9.0)).astype(np.uint16)   # even count, small
    cases["tiny_u16_k3_d2"] = (even_small, 3.0, 2)
    return cases


def segmentation_cases():
    """name -> (labels, dilate) for make_segmentation_mask."""
    rng = np.random.default_rng(202)
    labels = np.zeros((24, 30, 28), dtype=np.int32)
    labels[rng.random(labels.shape) < 0.004] = 7
    labels[0, :, 0] = 3            # on edges
    labels[23, 29, 27] = 9         # corner
    labels[10:13, 4:20, 5] = -4    # negative ids are background
    return {f"seg_d{d}": (labels, d) for d in (0, 1, 2)}


def skeleton_cases():
    """name -> (points, start, patch_shape, dilate) for make_skeleton_mask."""
    rng = np.random.default_rng(303)
    start = np.array([100, 200, 300])
    shape = (20, 24, 16)
    t = np.linspace(-5, 30, 400)
    pts = np.stack([100 + 0.6 * t, 200 + 0.8 * t + 0.3 * np.sin(t), 300 + 0.45 * t], axis=1)
    pts = pts + rng.uniform(-0.4, 0.4, pts.shape)     # float points, some outside the patch
    pts = np.concatenate([pts, [[99.99, 205.0, 305.0], [120.0, 210.0, 301.0], [110.0, 223.999, 315.5]]])
    return {f"skel_d{d}": (pts, start, shape, d) for d in (0, 1, 2)}


def score_cases():
    """name -> (raw, mask) for local_autocorr (lags 1, 2, 3) and highfreq_energy_fraction."""
    rng = np.random.default_rng(404)
    cases = {}
    blob = smooth_blob()
    cases["blob"] = (blob, blob > 50)
    sp, region = salt_pepper()
    cases["salt_pepper"] = (sp, region)
    big = np.full(GATE_SHAPE, 60000.0) + rng.integers(-2, 3, GATE_SHAPE)   # |mean| >> std
    m = np.zeros(GATE_SHAPE, dtype=bool)
    m[4:36, 4:36, 6:34] = True
    cases["offset_60000"] = (big.astype(np.float32), m)
    const = np.full(GATE_SHAPE, 123.25, dtype=np.float32)
    cases["constant"] = (const, m)
    border = (_background(rng, GATE_SHAPE, 10.0, 3.0) + _tube(GATE_SHAPE, axis=2, center=(0.0, 39.0))).astype(np.float32)
    bm = np.zeros(GATE_SHAPE, dtype=bool)
    bm[:6, 34:, :] = True
    bm[:, 0, 0] = True
    cases["border_tube"] = (border, bm)
    u16 = np.rint(_background(rng, GATE_SHAPE, 200.0, 20.0)).astype(np.uint16)
    cases["u16_noise_border"] = (u16, rng.random(GATE_SHAPE) < 0.3)
    return cases


def gate_cases():
    """name -> (labels, raw, min_segment_voxels) for patch_has_incoherent_segment."""
    rng = np.random.default_rng(505)
    cases = {}
    blob = smooth_blob()
    lab = np.zeros(GATE_SHAPE, dtype=np.uint64)
    lab[blob > 50] = 11
    cases["blob_kept"] = (lab, blob, 50)
    sp, region = salt_pepper()
    lab = np.zeros(GATE_SHAPE, dtype=np.uint64)
    lab[region] = 5
    cases["salt_pepper_flagged"] = (lab, sp, 50)
    cases["empty"] = (np.zeros(GATE_SHAPE, dtype=np.uint64), sp, 50)
    sp27, reg27 = salt_pepper(lo=20, hi=23)
    lab = np.zeros(GATE_SHAPE, dtype=np.uint32)
    lab[reg27] = 2
    cases["speck_27_ignored"] = (lab, sp27, 50)
    # uint64 ids above 2^32: a coherent blob and an incoherent block side by side
    raw = blob.copy()
    sp2, reg2 = salt_pepper(lo=33, hi=40, seed=3)
    raw[reg2] = sp2[reg2]
    lab = np.zeros(GATE_SHAPE, dtype=np.uint64)
    lab[blob > 50] = (1 << 40) + 17
    lab[reg2] = (1 << 33) + 1
    cases["u64_big_ids"] = (lab, raw, 50)
    lab2 = lab.copy()
    lab2[reg2] = 0
    cases["u64_big_ids_blob_only"] = (lab2, raw, 50)
    # int32 with negative ids: the incoherent block is labelled -5 (background), the blob 4
    lab = np.zeros(GATE_SHAPE, dtype=np.int32)
    lab[blob > 50] = 4
    lab[reg2] = -5
    cases["i32_negative_ids"] = (lab, raw, 50)
    # several segments per patch, mixed sizes
    lab = rng.integers(0, 12, GATE_SHAPE).astype(np.int64)
    noise = (_background(rng, GATE_SHAPE, 300.0, 40.0)).astype(np.float32)
    cases["many_noise_segments"] = (lab, noise, 50)
    # 20000 distinct labels: more than the device set holds (host path); one big incoherent block
    lab = np.zeros(GATE_SHAPE, dtype=np.uint64)
    outside = np.flatnonzero(~region.reshape(-1))
    lab.reshape(-1)[rng.permutation(outside)[:19999]] = np.arange(1, 20000, dtype=np.uint64) + 1000
    lab[region] = 7
    cases["overflow_20000"] = (lab, sp, 50)
    return cases


def gate_batch():
    """Every gate case as one batch (labels widened to int64, raw float32), for the batched form."""
    cases = gate_cases()
    names = list(cases)
    labels = np.stack([cases[n][0].astype(np.int64) for n in names])
    raw = np.stack([cases[n][1].astype(np.float32) for n in names])
    return names, labels, raw


def segment_stats_np(raw, mask, lag, smooth=None):
    """The 23 columns of exabm4d_segment_stats_dev for one mask, in numpy (two-pass, centred)."""
    raw = np.asarray(raw, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    v = raw[mask]
    n = float(v.size)
    row = [n, v.mean() if n else 0.0, 0.0, 0.0, 0.0]
    if smooth is not None and n:
        h = (raw - smooth)[mask]
        row[2] = h.mean()
        row[4] = float(np.sum((h - h.mean()) ** 2))
    if n:
        row[3] = float(np.sum((v - v.mean()) ** 2))
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -lag)
        hi[ax] = slice(lag, None)
        sel = mask[tuple(lo)] & mask[tuple(hi)]
        x = raw[tuple(lo)][sel]
        y = raw[tuple(hi)][sel]
        if x.size:
            dx, dy = x - x.mean(), y - y.mean()
            row += [float(x.size), x.mean(), y.mean(), float(np.sum(dx * dx)), float(np.sum(dy * dy)),
                    float(np.sum(dx * dy))]
        else:
            row += [0.0] * 6
    return np.array(row, dtype=np.float64)


def inputs_digest():
    """sha256 over every regenerated input, in a fixed order (stored in the fixture)."""
    import hashlib
    h = hashlib.sha256()
    groups = [foreground_cases(), segmentation_cases(), skeleton_cases(), score_cases(), gate_cases()]
    for cases in groups:
        for name in cases:
            h.update(name.encode())
            for a in cases[name]:
                a = np.ascontiguousarray(a)
                h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()
