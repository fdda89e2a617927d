"""The five kernel families of csrc/mask_kernels.hip, called through _native.Context, against the plain
references of tests/mask_pyref.py: radix-select threshold and foreground mask, binary dilation, the fp64
Gaussian, the LDS label set and the two-pass segment statistics.

Every device operand lives in a util.GuardedView: byte masks at odd element offsets, doubles one element past
16-byte alignment, a guard band on both sides that must come back as uploaded, inputs checked untouched.
Everything integer or bit-defined is compared for equality; the float columns of the segment statistics within
mask_pyref.segment_stats_bound, which is derived from the number format and not from the kernel; every case
prints its error / bound ratio (run with -s) and the last test the largest."""
import numpy as np
import pytest

import mask_pyref as P
from util import GuardedView

from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression.machine_learning import metrics

pytestmark = pytest.mark.gpu

BIG_BATCH, BIG_SHAPE = 65, (64, 64, 64)       # 17 039 360 voxels: more than 65536 workgroups of 256 threads
LABEL_TYPES = [np.uint8, np.uint32, np.uint64, np.int32, np.int64]
RATIOS = {}


def free_all(*views):
    for v in views:
        if v is not None:
            v.free()


def same_bits_or_nan(got, want, what):
    """fp32 thresholds: NaN where the reference is NaN, the same bits elsewhere."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN thresholds")
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32), err_msg=f"{what}: threshold bits")


# ---- threshold and foreground mask -------------------------------------------------------------------------
def fg_run(ctx, batch, k, dilate, what=""):
    """foreground_masks of a (B, z, y, x) batch, checked against the reference patch by patch."""
    batch = np.ascontiguousarray(batch)
    b, shape = batch.shape[0], batch.shape[1:]
    src = GuardedView(ctx, batch.dtype, batch.size, 1, batch)
    out = GuardedView(ctx, np.uint8, batch.size, 3)
    try:
        thr = ctx.foreground_masks(src.ptr, batch.dtype, b, shape, k, dilate, out.ptr)
        same_bits_or_nan(thr, [P.fg_threshold(p, k) for p in batch], what)
        want = np.stack([P.fg_mask(p, k, dilate) for p in batch])
        out.check_output(want.astype(np.uint8), what)
        src.check_untouched(what)
    finally:
        free_all(src, out)
    return thr, want


def shape_of(n):
    return {64 ** 3: (64, 64, 64), 37 * 64 * 50: (37, 64, 50)}.get(n, (1, 1, n))


def fg_kinds(dtype, n, seed):
    """name -> n values: the data at which a radix selection goes wrong."""
    rng = np.random.default_rng(seed)
    lo, hi = n // 2, n - n // 2
    if dtype == np.uint16:
        kinds = {
            "noise": rng.integers(900, 1100, n),
            "equal": np.full(n, 777),
            "split": rng.permutation(np.r_[np.full(lo, 40), np.full(hi, 41000)]),    # the median sits on the split
            "ties": rng.integers(1000, 1004, n),
            "ends": rng.choice([0, 0, 65535, 65535, 300], n),
            "ends_rare": np.where(rng.random(n) < 0.1, rng.choice([0, 65535], n), rng.integers(30000, 30050, n)),
        }
    else:
        low_byte = (np.uint32(0x42C81200) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
        signed = rng.choice(np.array([-3.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 2.0, -1e30, 7e-39], np.float32), n)
        infs = rng.normal(50.0, 9.0, n)
        infs[rng.random(n) < 0.05] = np.inf
        infs[rng.random(n) < 0.05] = -np.inf
        kinds = {
            "noise": rng.normal(100.0, 20.0, n),
            "equal": np.full(n, -12.625),
            "split": rng.permutation(np.r_[np.full(lo, -1.5), np.full(hi, 2.25)]),
            "low_byte": low_byte,                       # keys that share their top three bytes
            "signed_denormal": signed,
            "negative": rng.normal(-4000.0, 3.0, n),
            "infinities": infs,
        }
    return {name: np.asarray(v).astype(dtype) for name, v in kinds.items()}


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 64 ** 3, 37 * 64 * 50])
def test_threshold_and_mask(ctx, dtype, n):
    """Ragged last waves around the one-add-of-64 shortcut, n < 64, tied medians, keys that differ in the lowest
    byte only, negatives, signed zeros, denormals, infinities, uint16's ends; k exact and inexact in fp32."""
    for name, v in fg_kinds(dtype, n, n).items():
        for k in (0.0, 2.7, 3.0, 6.0):
            fg_run(ctx, v.reshape((1,) + shape_of(n)), k, 1 if k == 3.0 else 0, f"{np.dtype(dtype)} n={n} {name} k={k}")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_threshold_of_each_patch_of_a_batch(ctx, dtype):
    """Six patches at widely different levels: every patch gets ITS threshold (thr[i / n]), in either order, and
    equals its single-patch call."""
    rng = np.random.default_rng(5)
    shape = (6, 7, 9)
    levels = [3.0, 40.0, 900.0, 20000.0, 150.0, 60000.0] if dtype == np.uint16 else [1e-3, 1.0, -1e6, 1e20, 100.0, 1e4]
    batch = np.stack([(lv + abs(lv) * 0.01 * rng.normal(0, 1, shape) + abs(lv) * 0.5 * (rng.random(shape) < 0.05))
                      for lv in levels])
    batch = (np.rint(batch.clip(0, 65535)) if dtype == np.uint16 else batch).astype(dtype)
    for dilate in (0, 2):
        thr, masks = fg_run(ctx, batch, 3.0, dilate, "forwards")
        assert len(set(thr.tolist())) == len(levels) and all(m.any() for m in masks)
        thr_r, masks_r = fg_run(ctx, batch[::-1], 3.0, dilate, "reversed")
        assert np.array_equal(thr_r[::-1].view(np.uint32), thr.view(np.uint32)) and np.array_equal(masks_r[::-1], masks)
        for b in range(len(levels)):
            t1, m1 = fg_run(ctx, batch[b:b + 1], 3.0, dilate, f"patch {b} alone")
            assert t1.view(np.uint32)[0] == thr.view(np.uint32)[b] and np.array_equal(m1[0], masks[b])


def _nan_patch(seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(30.0, 4.0, (5, 6, 7)) + 200.0 * (rng.random((5, 6, 7)) < 0.05)).astype(np.float32)


@pytest.mark.parametrize("dilate", [0, 2])
def test_nan_propagates_as_in_numpy(ctx, dilate):
    """np.median of data that holds a NaN is NaN: the threshold is NaN and the mask empty, also after dilation.
    The same wherever numpy's own arithmetic gives NaN: an infinite median makes |raw - med| hold inf - inf."""
    neg_nan = np.uint32(0xFFC00001).view(np.float32)
    cases = {}
    for name, bad in (("one_nan", np.nan), ("negative_nan", neg_nan)):
        p = _nan_patch(1)
        p[2, 3, 4] = bad
        cases[name] = p
        q = _nan_patch(2)
        q.reshape(-1)[[0, -1]] = bad            # first and last voxel
        cases[name + "_ends"] = q
    cases["all_nan"] = np.full((5, 6, 7), np.nan, np.float32)
    cases["all_negative_nan"] = np.full((5, 6, 7), neg_nan, np.float32)
    p = _nan_patch(3)
    p[:3] = np.inf
    cases["median_plus_inf"] = p
    cases["median_minus_inf"] = -p
    p = _nan_patch(4)
    p.reshape(-1)[:105] = -np.inf
    p.reshape(-1)[105:] = np.inf                # even count: the median is (-inf + inf) / 2
    cases["median_of_both_infinities"] = p
    for name, p in cases.items():
        thr, masks = fg_run(ctx, p[None], 6.0, dilate, name)
        assert np.isnan(thr[0]) and not masks.any(), name
    # a NaN in patch 2 of 4 only: the other three are what they are alone
    batch = np.stack([_nan_patch(10 + b) for b in range(4)])
    clean_thr, clean_masks = fg_run(ctx, batch, 6.0, dilate, "clean batch")
    batch[2, 4, 5, 6] = np.nan
    thr, masks = fg_run(ctx, batch, 6.0, dilate, "NaN in patch 2")
    assert np.isnan(thr[2]) and not masks[2].any()
    keep = [0, 1, 3]
    assert np.array_equal(thr[keep].view(np.uint32), clean_thr[keep].view(np.uint32))
    assert np.array_equal(masks[keep], clean_masks[keep]) and all(masks[b].any() for b in keep)


# ---- dilation -----------------------------------------------------------------------------------------------
def dilate_run(ctx, batch, iterations, what=""):
    batch = np.ascontiguousarray(batch, dtype=np.uint8)
    src = GuardedView(ctx, np.uint8, batch.size, 1, batch)
    out = GuardedView(ctx, np.uint8, batch.size, 3)
    try:
        ctx.binary_dilate(src.ptr, batch.shape[0], batch.shape[1:], iterations, out.ptr)
        want = np.stack([P.dilate(p, iterations) for p in batch])
        out.check_output(want.astype(np.uint8), what)
        src.check_untouched(what)
    finally:
        free_all(src, out)
    return want


def seed_sets(shape, seed):
    """Four patches of seeds: every corner; the middle of every edge; the centre of every face; random non-0
    bytes other than 1."""
    nz, ny, nx = shape
    ends = [sorted({0, s - 1}) for s in shape]
    mid = [s // 2 for s in shape]
    sets = np.zeros((4,) + shape, dtype=np.uint8)
    for z in ends[0]:
        for y in ends[1]:
            for x in ends[2]:
                sets[0, z, y, x] = 1
            sets[1, z, y, mid[2]] = 1
        for x in ends[2]:
            sets[1, z, mid[1], x] = 1
        sets[2, z, mid[1], mid[2]] = 1
    for y in ends[1]:
        for x in ends[2]:
            sets[1, mid[0], y, x] = 1
        sets[2, mid[0], y, mid[2]] = 1
    for x in ends[2]:
        sets[2, mid[0], mid[1], x] = 1
    rng = np.random.default_rng(seed)
    sets[3] = (rng.random(shape) < 0.06) * rng.integers(2, 256, shape)
    return sets


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (2, 1, 5), (1, 7, 2), (2, 2, 2), (5, 2, 1), (3, 4, 5), (9, 12, 7)])
def test_dilation_iterations_and_thin_axes(ctx, shape):
    """Iterations 0 .. 8 (both parities of the ping-pong, well past 5) on axes of 1 and 2 voxels, seeds on every
    corner, edge and face, bytes other than 1; four patches side by side in one call."""
    sets = seed_sets(shape, sum(shape))
    for iterations in range(9):
        dilate_run(ctx, sets, iterations, f"{shape} x{iterations}")
        dilate_run(ctx, sets[::-1], iterations, f"{shape} reversed x{iterations}")


@pytest.mark.parametrize("shape", [(4, 5, 6), (1, 1, 8), (3, 1, 1)])
def test_dilation_does_not_cross_patches(ctx, shape):
    batch = np.zeros((5,) + shape, dtype=np.uint8)
    batch[1] = batch[3] = 1                       # full patches between empty ones
    for iterations in range(1, 5):
        want = dilate_run(ctx, batch, iterations, f"{shape} x{iterations}")
        assert np.array_equal(want, batch != 0)
        if batch[0].size < 5:
            continue
        fg = np.ones(batch.shape, dtype=np.float32)                 # the same through the fused first pass:
        fg[1::2, 0, 0, 0] = fg[1::2, -1, -1, -1] = 9.0              # foreground on the two ends of patches 1 and 3
        _, masks = fg_run(ctx, fg, 0.0, iterations, f"{shape} fused x{iterations}")
        assert masks[1, 0, 0, 0] and masks[3, -1, -1, -1] and not masks[::2].any()


def test_dilation_refuses_in_place(ctx):
    g = GuardedView(ctx, np.uint8, 60, 1, np.ones(60, np.uint8))
    try:
        with pytest.raises(ValueError):
            ctx.binary_dilate(g.ptr, 1, (3, 4, 5), 1, g.ptr)
        g.check_untouched()
    finally:
        g.free()


def test_dilation_grid_stride(ctx):
    """65 patches of 64^3: every thread takes a second voxel, and the patch boundary 64 * 64^3 falls inside the
    second stride.  Seeds on the first and last voxel of every patch would show across it."""
    rng = np.random.default_rng(65)
    batch = (rng.random((BIG_BATCH,) + BIG_SHAPE) < 0.004).astype(np.uint8)
    batch[:, 0, 0, 0] = batch[:, -1, -1, -1] = 1
    batch[::2, 0, 0, 0] = 0
    for iterations in (1, 2):
        dilate_run(ctx, batch, iterations, f"x{iterations}")


# ---- Gaussian -----------------------------------------------------------------------------------------------
def gauss_run(ctx, batch, weights, what=""):
    batch = np.ascontiguousarray(batch)
    src = GuardedView(ctx, batch.dtype, batch.size, 1, batch)
    out = GuardedView(ctx, np.float64, batch.size, 1)
    try:
        ctx.gaussian_filter3d(src.ptr, batch.dtype, batch.shape[0], batch.shape[1:], weights, out.ptr)
        want = np.stack([P.gaussian(p, weights) for p in batch])
        out.check_output(want, what)
        src.check_untouched(what)
    finally:
        free_all(src, out)
    return want


@pytest.mark.parametrize("sigma", [0.0, 0.5, 1.0, 2.0, 3.7, 16.0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gaussian_bit_for_bit(ctx, dtype, sigma):
    """Radius 0 .. 64 (the maximum) on axes down to 1 voxel, so the reflection repeats many times; three patches
    with the middle one scaled by 1e6, where a read across a patch boundary shows at once."""
    w = metrics.gaussian_weights(sigma)
    rng = np.random.default_rng(int(sigma * 10) + np.dtype(dtype).itemsize)
    for shape in [(1, 1, 1), (1, 2, 3), (5, 19, 3), (13, 17, 11), (3, 3, 200)]:
        batch = rng.normal(100.0, 15.0, (3,) + shape)
        batch[1] *= 1e6
        want = gauss_run(ctx, batch.astype(dtype), w, f"sigma {sigma} {shape}")
        assert want[0].max() < 1e3 and want[2].max() < 1e3 and want[1].min() > 1e6


def test_gaussian_refusals(ctx):
    src = GuardedView(ctx, np.float64, 60, 1, np.ones(60))
    out = GuardedView(ctx, np.float64, 60, 1)
    try:
        with pytest.raises(ValueError):
            ctx.gaussian_filter3d(src.ptr, np.float64, 1, (3, 4, 5), np.full(66, 1.0 / 131.0), out.ptr)   # radius 65
        with pytest.raises(ValueError):
            ctx.gaussian_filter3d(src.ptr, np.float64, 1, (3, 4, 5), metrics.gaussian_weights(1.0), src.ptr)
        ctx.gaussian_filter3d(src.ptr, np.float64, 1, (3, 4, 5), np.r_[1.0, np.zeros(64)], out.ptr)       # radius 64
        out.check_output(np.ones(60))
        src.check_untouched()
    finally:
        free_all(src, out)


def test_gaussian_grid_stride(ctx):
    rng = np.random.default_rng(66)
    batch = rng.normal(100.0, 30.0, (BIG_BATCH,) + BIG_SHAPE).astype(np.float32)
    batch[1::2] *= 1e3
    gauss_run(ctx, batch, metrics.gaussian_weights(1.0), "65 x 64^3")


# ---- label set ----------------------------------------------------------------------------------------------
def label_ids(dtype, count, rng):
    """`count` distinct positive ids of the type, its largest ones among them."""
    top = {np.uint8: [255], np.uint32: [2 ** 32 - 1, 2 ** 31], np.uint64: [2 ** 64 - 1, 2 ** 63, 2 ** 32],
           np.int32: [2 ** 31 - 1], np.int64: [2 ** 63 - 1, 2 ** 32 + 1]}[dtype][:count]
    hi = min(int(np.iinfo(dtype).max), 2 ** 62)
    ids = set(top)
    if hi == 255:
        ids.update(int(v) for v in rng.permutation(np.arange(1, 255))[:count - len(ids)])
    while len(ids) < count:
        ids.update(int(v) for v in rng.integers(1, hi, count - len(ids), dtype=np.uint64))
    return np.array(sorted(ids), dtype=dtype)


def label_run(ctx, labels, shape, what=""):
    """label_set and metrics._label_lists of one patch: (keys sorted, counts, held, status)."""
    labels = np.ascontiguousarray(labels).reshape((1,) + shape)
    g = GuardedView(ctx, labels.dtype, labels.size, 1, labels)
    try:
        keys, counts, held, status = ctx.label_set(g.ptr, labels.dtype, 1, shape)
        lists = metrics._label_lists(ctx, g.ptr, labels, 1, shape)
        g.check_untouched(what)
    finally:
        g.free()
    u, c = P.label_counts(labels)
    np.testing.assert_array_equal(lists[0][0], u.astype(np.uint64), err_msg=f"{what}: label list")
    np.testing.assert_array_equal(lists[0][1], c, err_msg=f"{what}: label counts")
    assert held[0] <= nat.LABEL_SET_MAX and status[0] in (0, 1), what
    if status[0] == 0:
        order = np.argsort(keys[0, :held[0]])
        np.testing.assert_array_equal(keys[0, :held[0]][order], u.astype(np.uint64), err_msg=f"{what}: set")
        np.testing.assert_array_equal(counts[0, :held[0]][order], c, err_msg=f"{what}: set counts")
    return int(held[0]), int(status[0])


def background(dtype, n, rng):
    if np.dtype(dtype).kind == "u":
        return np.zeros(n, dtype)
    return rng.choice(np.array([0, -1, np.iinfo(dtype).min, -77], dtype=dtype), n)


@pytest.mark.parametrize("dtype", LABEL_TYPES)
@pytest.mark.parametrize("distinct", [1, 512, 1023, 1024, 1025, 20000])
def test_label_set_at_its_capacity(ctx, dtype, distinct):
    """Status 0 and the exact set up to EXABM4D_LABEL_SET_MAX distinct labels, status 1 above, the label list
    np.unique's in every case.  Every label at least 3 times, shuffled, ids at the ends of the type, the most
    negative id as background, n no multiple of 1024."""
    if dtype == np.uint8 and distinct > 255:
        distinct = {512: 254, 1023: 255}.get(distinct)
        if distinct is None:
            return
    for seed in range(4):
        rng = np.random.default_rng(1000 * distinct + seed)
        ids = label_ids(dtype, distinct, rng)
        assert len(np.unique(ids)) == distinct
        v = np.r_[np.repeat(ids, 3), rng.choice(ids, 50), background(dtype, 137 + seed, rng)].astype(dtype)
        rng.shuffle(v)
        assert v.size % 1024
        held, status = label_run(ctx, v, (1, 1, v.size), f"{np.dtype(dtype)} {distinct} labels seed {seed}")
        assert status == (1 if distinct > nat.LABEL_SET_MAX else 0), (np.dtype(dtype), distinct, seed, held)
        if not status:
            assert held == distinct


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64, np.int64])
def test_label_set_filled_by_a_label_many_threads_meet_at_once(ctx, dtype):
    """Exactly EXABM4D_LABEL_SET_MAX labels, the last of them first met by hundreds of threads of one sweep: one
    claims the slot and fills the set, the others saw the slot empty and then see the set full.  The key is
    held, not new: status 0."""
    for seed in range(6):
        rng = np.random.default_rng(seed)
        ids = label_ids(dtype, nat.LABEL_SET_MAX, rng)
        rng.shuffle(ids)
        head = np.repeat(ids[:-1], 3)
        head = np.r_[head, rng.choice(ids[:-1], -head.size % 1024)].astype(dtype)    # whole sweeps of 1024 threads
        rng.shuffle(head)
        assert len(np.unique(head)) == nat.LABEL_SET_MAX - 1
        tail = np.where(np.arange(1024) % 2 == 0, ids[-1], rng.choice(ids[:-1], 1024)).astype(dtype)
        v = np.r_[head, tail, np.repeat(ids[:5], 3)].astype(dtype)
        held, status = label_run(ctx, v, (1, 1, v.size), f"{np.dtype(dtype)} seed {seed}")
        assert (held, status) == (nat.LABEL_SET_MAX, 0), (np.dtype(dtype), seed, held, status)


@pytest.mark.parametrize("dtype", LABEL_TYPES)
@pytest.mark.parametrize("offset", [0, 1])
def test_label_set_runs_of_64(ctx, dtype, offset):
    """Runs of 64 equal labels: aligned to a wave they take the one-insert-of-64 path, offset by one voxel every
    wave holds two labels."""
    rng = np.random.default_rng(64 + offset)
    ids = label_ids(dtype, 40, rng)
    runs = np.repeat(rng.choice(ids, 70), 64)
    runs[64 * 7:64 * 8] = background(dtype, 64, rng)[0]           # a whole wave of background
    v = np.r_[background(dtype, offset, rng), runs, ids[:3]].astype(dtype)
    held, status = label_run(ctx, v, (1, 1, v.size), f"{np.dtype(dtype)} offset {offset}")
    assert status == 0 and held == len(np.unique(v[v > 0]))


# ---- segment statistics -------------------------------------------------------------------------------------
def seg_run(ctx, labels, raw, smooth, lag, items, what=""):
    """segment_stats of (B, z, y, x) operands for `items` = [(patch, key)], each row against the exact columns
    within the derived bound; returns the rows."""
    labels, raw = np.ascontiguousarray(labels), np.ascontiguousarray(raw)
    b, shape = labels.shape[0], labels.shape[1:]
    gl = GuardedView(ctx, labels.dtype, labels.size, 1, labels)
    gr = GuardedView(ctx, raw.dtype, raw.size, 1, raw)
    gs = GuardedView(ctx, np.float64, raw.size, 1, smooth) if smooth is not None else None
    try:
        got = ctx.segment_stats(gl.ptr, labels.dtype, gr.ptr, raw.dtype, gs.ptr if gs else None, b, shape, lag,
                                [p for p, _ in items], np.array([k for _, k in items], dtype=np.uint64))
        for g in (gl, gr, gs):
            if g is not None:
                g.check_untouched(what)
    finally:
        free_all(gl, gr, gs)
    assert got.shape == (len(items), nat.SEG_STATS_K)
    worst = 0.0
    for row, (p, key) in zip(got, items):
        sm = smooth[p] if smooth is not None else None
        want = P.segment_stats_exact(labels[p], key, raw[p], lag, sm)
        bound = P.segment_stats_bound(labels[p], key, raw[p], lag, sm)
        worst = max(worst, P.check_stats(row, want, bound, f"{what} patch {p} key {key} lag {lag}"))
    RATIOS[what] = max(RATIOS.get(what, 0.0), worst)
    print(f"error / bound {worst:.2e}  {what} lag {lag}")
    return got


def smooth_of(raw):
    return np.stack([P.gaussian(p, metrics.gaussian_weights(1.0)) for p in raw])


def three_segments(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    ids = label_ids(dtype, 3, rng)
    pick = rng.integers(0, 5, shape)                              # 0 and 4: background
    labels = np.zeros(shape, dtype=dtype)
    for j in range(3):
        labels[pick == j + 1] = ids[j]
    if np.dtype(dtype).kind == "i":
        labels[pick == 4] = np.iinfo(dtype).min
    labels[0, 0, :] = ids[0]                                      # a full row, so long lags have pairs
    labels[:, 0, 0] = ids[1]
    return labels, [int(i) for i in ids]


@pytest.mark.parametrize("rdt", [np.float32, np.float64])
@pytest.mark.parametrize("ldt", LABEL_TYPES)
def test_segment_stats_every_type_pair_and_lag(ctx, ldt, rdt):
    """All 23 columns of all ten instantiations on a 12 x 9 x 20 patch with three segments; lags up to and past
    the length of an axis (len - 1, len, more); smooth NULL (zero columns) and given."""
    shape = (12, 9, 20)
    labels, ids = three_segments(ldt, shape, 3)
    rng = np.random.default_rng(7)
    raw = (rng.normal(300.0, 40.0, shape) + 5.0 * np.arange(20)).astype(rdt)
    smooth = smooth_of(raw[None])
    items = [(0, k) for k in ids]
    for lag in (1, 2, 3, 8, 9, 19, 20, 25):
        got = seg_run(ctx, labels[None], raw[None], None, lag, items, f"{np.dtype(ldt)}/{np.dtype(rdt)}")
        assert not got[:, [2, 4]].any()
        assert got[:, 5].any() == (lag < 12) and got[:, 11].any() == (lag < 9) and got[:, 17].any() == (lag < 20)
        seg_run(ctx, labels[None], raw[None], smooth, lag, items, f"{np.dtype(ldt)}/{np.dtype(rdt)} smooth")


def test_segment_stats_pairs_do_not_wrap(ctx):
    """Segment 1 holds the last voxel of every row and the first of the next, segment 2 the last row of every
    plane and the first of the next, segment 3 the last plane of patch 0 and the first of patch 1: a pair
    that wraps over a row, plane or patch end would count.  The last patch of the batch carries no item."""
    shape = (6, 5, 8)
    rng = np.random.default_rng(11)
    raw = rng.normal(50.0, 10.0, (3,) + shape)
    labels = np.zeros((3,) + shape, dtype=np.int32)
    labels[:2, :, :, 0] = labels[:2, :, :, -1] = 1
    labels[:2, :, 0, 1:-1] = labels[:2, :, -1, 1:-1] = 2
    labels[0, -1, 1:-1, 1:-1] = labels[1, 0, 1:-1, 1:-1] = 3
    labels[2] = labels[1]
    items = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]
    for lag in (1, 2, 4, 5, 6):
        got = seg_run(ctx, labels, raw.astype(np.float32), None, lag, items, "row, plane and patch ends")
        if lag == 1:
            assert got[0, 17] == 0 and got[1, 11] == 0 and got[2, 5] == 0     # the only candidates would wrap


@pytest.mark.parametrize("shape", [(1, 1, 40), (40, 1, 1), (1, 40, 1)])
def test_segment_stats_thin_patches(ctx, shape):
    rng = np.random.default_rng(40)
    labels = rng.integers(0, 3, (2,) + shape).astype(np.uint8)
    raw = rng.normal(10.0, 3.0, (2,) + shape)
    for lag in (1, 2, 3, 39, 40, 45):
        seg_run(ctx, labels, raw, smooth_of(raw), lag, [(0, 1), (0, 2), (1, 1)], f"thin {shape}")


def test_segment_stats_items(ctx):
    """Items of several patches that share a label id, out of order and duplicated; a key that no voxel has gives
    a row of zeros; a row does not depend on the items around it."""
    rng = np.random.default_rng(12)
    shape = (7, 8, 9)
    labels = rng.integers(0, 4, (4,) + shape).astype(np.uint64) * np.uint64(2 ** 40 + 5)
    raw = rng.normal(1000.0, 100.0, (4,) + shape).astype(np.float32)
    smooth = smooth_of(raw)
    k = 2 ** 40 + 5
    items = [(2, k), (0, 3 * k), (2, k), (1, k), (0, k), (2, 777), (1, 3 * k), (0, k), (2, 2 ** 64 - 1)]
    got = seg_run(ctx, labels, raw, smooth, 2, items, "items")
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[4], got[7])
    assert not got[5].any() and not got[8].any() and got[[0, 1, 3, 4, 6], 0].all()
    for j, item in enumerate(items):
        assert np.array_equal(seg_run(ctx, labels, raw, smooth, 2, [item], "items, one at a time")[0], got[j])


def test_segment_stats_hostile_means(ctx):
    """|mean| >> sd: float32 at 60 000 +- 0.5 and float64 at 1e9 +- 1.  A one-pass sum r^2 - n m^2 misses the
    bound by orders of magnitude here."""
    rng = np.random.default_rng(13)
    shape = (12, 9, 20)
    labels = rng.integers(0, 3, (2,) + shape).astype(np.int64)
    for name, raw in (("float32 at 60000", rng.normal(60000.0, 0.5, (2,) + shape).astype(np.float32)),
                      ("float64 at 1e9", rng.normal(1e9, 1.0, (2,) + shape))):
        for lag in (1, 3):
            seg_run(ctx, labels, raw, smooth_of(raw), lag, [(0, 1), (0, 2), (1, 1), (1, 2)], name)
        v = raw[0][labels[0] == 1].astype(np.float64)
        one_pass = float(np.sum(v * v) - v.size * v.mean() ** 2)
        want, bound = P.segment_stats_exact(labels[0], 1, raw[0], 1), P.segment_stats_bound(labels[0], 1, raw[0], 1)
        assert abs(one_pass - want[3]) > 100 * bound[3], name


def test_segment_stats_refuses_key_zero(ctx):
    """label_key maps every background voxel to 0, so key 0 would select the background; the header says labels
    <= 0 never belong to a segment.  Refused, among other items too."""
    labels = np.zeros((1, 3, 4, 5), dtype=np.int32)
    labels[0, 1] = 4
    raw = np.ones((1, 3, 4, 5), dtype=np.float32)
    gl, gr = GuardedView(ctx, np.int32, 60, 1, labels), GuardedView(ctx, np.float32, 60, 1, raw)
    try:
        for keys in ([0], [4, 0], [0, 4]):
            with pytest.raises(ValueError):
                ctx.segment_stats(gl.ptr, np.int32, gr.ptr, np.float32, None, 1, (3, 4, 5), 1, [0] * len(keys), keys)
        assert ctx.segment_stats(gl.ptr, np.int32, gr.ptr, np.float32, None, 1, (3, 4, 5), 1, [0], [4])[0, 0] == 20
    finally:
        free_all(gl, gr)


# ---- end to end ---------------------------------------------------------------------------------------------
def score_bounds(st, bound):
    """What the column bounds allow the two finished scores to move, to first order, plus 1e-15 for the handful
    of roundings of the finishing rules themselves: c = Sxy / sqrt(Sxx Syy) moves by at most
    b_xy / sqrt(Sxx Syy) + |c| (b_xx / Sxx + b_yy / Syy) / 2 per axis (the mean over axes by no more than the
    largest), and h = SS_hf / SS_raw by (b_hf + h b_raw) / SS_raw."""
    ac = 0.0
    for ax in range(3):
        n, _, _, sxx, syy, sxy = st[5 + 6 * ax:11 + 6 * ax]
        if n >= 2 and sxx > 0 and syy > 0:
            root = np.sqrt(sxx * syy)
            b = bound[5 + 6 * ax:11 + 6 * ax]
            ac = max(ac, b[5] / root + abs(sxy) / root * (b[3] / sxx + b[4] / syy) / 2)
    hf = (bound[4] + st[4] / st[3] * bound[3]) / st[3] if st[3] > 0 else 0.0
    return 2 * ac + 1e-15, 2 * hf + 1e-15


@pytest.mark.parametrize("dtype", LABEL_TYPES)
def test_scores_and_gate_end_to_end(ctx, dtype):
    """segment_scores and incoherent_segments on random label volumes: the label lists are np.unique's, the
    scores the finishing rules applied to the exact statistics with mask_pyref's Gaussian, the decisions follow."""
    rng = np.random.default_rng(np.dtype(dtype).itemsize + (np.dtype(dtype).kind == "i"))
    shape = (10, 12, 14)
    ids = np.concatenate([np.zeros(1, dtype), label_ids(dtype, 4, rng)])
    labels = ids[rng.integers(0, 5, (3,) + shape)]
    labels[2] = ids[(np.arange(14) // 5 + 1)[None, None, :] * np.ones(shape, dtype=int)]      # three slabs
    zz = np.arange(10.0)[:, None, None]
    raw = (rng.normal(200.0, 30.0, (3,) + shape)).astype(np.float32)
    raw[2] = (200.0 + 40.0 * np.sin(zz / 3.0) + rng.normal(0, 1.0, shape)).astype(np.float32)   # smooth: coherent
    got = metrics.segment_scores(labels, raw, min_segment_voxels=50)
    flags = metrics.incoherent_segments(labels, raw, min_segment_voxels=50)
    smooth = smooth_of(raw)
    for b in range(3):
        u, c = P.label_counts(labels[b])
        keep = c >= 50
        assert [(s[0], s[1]) for s in got[b]] == [(int(k), int(n)) for k, n in zip(u[keep], c[keep])]
        flagged = False
        for (key, _, ac, hf) in got[b]:
            st = P.segment_stats_exact(labels[b], key, raw[b], 2, smooth[b])
            tol_ac, tol_hf = score_bounds(st, P.segment_stats_bound(labels[b], key, raw[b], 2, smooth[b]))
            want_ac, want_hf = metrics.autocorr_from_stats(st), metrics.highfreq_from_stats(st)
            assert abs(ac - want_ac) <= tol_ac and abs(hf - want_hf) <= tol_hf, (b, key, ac, want_ac, hf, want_hf)
            assert abs(want_ac - 0.4) > 1e-6 and abs(want_hf - 0.35) > 1e-6      # the inputs decide clearly
            flagged |= (not want_ac >= 0.4) and want_hf > 0.35
        assert bool(flags[b]) == flagged, b
    assert flags[0] and not flags[2]


def test_float32_raw_widens_on_the_device_as_on_the_host(ctx):
    """The Gaussian of float32 raw and of the same values widened on the host are the same bits, and so are the
    statistics the kernel makes of either."""
    rng = np.random.default_rng(32)
    shape = (9, 10, 11)
    raw32 = rng.normal(500.0, 80.0, (2,) + shape).astype(np.float32)
    raw64 = raw32.astype(np.float64)
    w = metrics.gaussian_weights(1.0)
    s32, s64 = gauss_run(ctx, raw32, w, "float32 source"), gauss_run(ctx, raw64, w, "float64 source")
    assert np.array_equal(s32, s64)
    labels = rng.integers(0, 3, (2,) + shape).astype(np.uint32)
    items = [(0, 1), (1, 2)]
    a = seg_run(ctx, labels, raw32, s32, 2, items, "float32 raw")
    b = seg_run(ctx, labels, raw64, s64, 2, items, "float64 raw")
    assert np.array_equal(a, b)


def test_zz_report_the_largest_ratio():
    """Last in the file: the largest error / bound ratio of every statistics case above."""
    if RATIOS:
        worst = max(RATIOS, key=RATIOS.get)
        print(f"largest error / bound ratio: {RATIOS[worst]:.3e} ({worst})")
        assert RATIOS[worst] <= 1.0
