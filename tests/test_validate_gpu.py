"""Validation scoring on the device (csrc/validate_kernels.hip) against tests/validate_pyref.py and,
for the metric dictionaries, also against the reference's stored values (tests/golden/validate_batch.npz):
``Context.evaluate_batch`` with every operand in a util.GuardedView (odd element offsets, guard bands checked,
inputs untouched), ``metrics.evaluate_examples`` from host arrays and from CUDA tensors, ``train.validate``.

med, mad, thr, the rank values, the counts, the maxima and the metrics made of them must be the pyref's values
bit for bit (validate_pyref.same), NaN where it has NaN.  Sums and MAEs of two uint16 images are integers below
2^53 and must be equal; the others must lie within 2 m 2^-53 of the pyref's, m the number of terms: any order of
fp64 additions of non-negative terms is within (m - 1) 2^-53 relative of the true sum.  Every case prints its
largest error / bound ratio (run with -s)."""
import os

import numpy as np
import pytest

import validate_inputs as vi
import validate_pyref as P
from util import GuardedView

from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression.machine_learning import metrics

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validate_batch.npz")
CASES = vi.all_cases()
_PYREF = {}
# row column -> pyref key, compared with validate_pyref.same
SAME = {2: "n_fg", 3: "n_bright", 4: "max_pred", 5: "max_raw", nat.EVAL_MED: "med", nat.EVAL_MAD: "mad",
        nat.EVAL_THR: "thr", nat.EVAL_RAW_LO: "raw_lo", nat.EVAL_RAW_HI: "raw_hi", nat.EVAL_PRED_LO: "pred_lo",
        nat.EVAL_PRED_HI: "pred_hi"}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def pyref(name, pct):
    """The pyref rows of a case, computed once."""
    if (name, pct) not in _PYREF:
        _PYREF[name, pct] = P.examples(*CASES[name], pct)
    return _PYREF[name, pct]


def mask_bytes(mask):
    return (mask > 0.5 if mask.dtype.kind == "f" else mask.astype(bool)).astype(np.uint8)


def ranks_of(n, pct):
    return [(n - 1) // 2, n // 2, *P.percentile_ranks(n, pct)]


def run_batch(ctx, case, pct, what=""):
    """Context.evaluate_batch on guarded, offset views of the case."""
    pred, raw, target, mask = case
    batch, n = pred.shape[0], int(np.prod(pred.shape[1:]))
    views = [GuardedView(ctx, a.dtype, a.size, k, a) for a, k in
             ((pred, 1), (raw, 3), (target, 1), (mask_bytes(mask), 3))]
    try:
        rows = ctx.evaluate_batch(views[0].ptr, pred.dtype, views[1].ptr, raw.dtype, views[2].ptr, target.dtype,
                                  views[3].ptr, batch, n, 6.0, ranks_of(n, pct))
        for v in views:
            v.check_untouched(what)
    finally:
        for v in views:
            v.free()
    return rows


def check_device_rows(rows, want_rows, case, what):
    """The (B, EVAL_K) rows against the pyref's; returns the largest error / bound ratio of the float sums."""
    pred, raw, target, _ = case
    u16 = P.u16_pairs(case)
    worst = 0.0
    for b, (row, want) in enumerate(zip(rows, want_rows)):
        for col, key in SAME.items():
            assert P.same(row[col], want[key]), f"{what} patch {b} {key}: {row[col]!r} != {want[key]!r}"
        for col, img in ((nat.EVAL_PRED_NAN, pred), (nat.EVAL_RAW_NAN, raw), (nat.EVAL_TARGET_NAN, target)):
            has_nan = img.dtype.kind == "f" and bool(np.isnan(img[b]).any())
            assert row[col] == float(has_nan), f"{what} patch {b}: NaN flag {col}"
        for col, key, terms, exact in ((0, "fg_sum", want["n_fg"], u16["fg_mae"]),
                                       (1, "bg_sum", want["n"] - want["n_fg"], u16["bg_mae"])):
            w = want[key]
            if exact or not np.isfinite(w) or w == 0.0:
                assert P.same(row[col], w), f"{what} patch {b} {key}: {row[col]!r} != {w!r}"
                continue
            ratio = abs(row[col] - w) / P.mae_bound(w, terms)
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{what} patch {b} {key}: {row[col]!r} vs {w!r}, error / bound = {ratio:.3g}"
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_metrics(ctx, golden, name):
    """Every shape x dtype combination and every content case, at pct 0 (virtual index n - 1), 0.1 and 50."""
    case = CASES[name]
    worst = 0.0
    for pct in vi.PCTS:
        what = f"{name} pct={pct:g}"
        want = pyref(name, pct)
        worst = max(worst, check_device_rows(run_batch(ctx, case, pct, what), want, case, what))
        got = metrics.evaluate_examples(*case, pct=pct)
        assert [tuple(g) for g in got] == [P.METRICS] * len(want)
        u16 = P.u16_pairs(case)
        want_values = np.array([[w[k] for k in P.METRICS] for w in want])
        worst = max(worst, P.check_rows(got, want_values, want, what + " vs pyref", u16))
        worst = max(worst, P.check_rows(got, golden[f"{name}/pct{pct:g}"], want, what + " vs reference", u16))
    print(f"\n{name}: largest sum / MAE error over bound {worst:.3g}")


@pytest.mark.parametrize("name", ["val_2x64x64x64", "f32_5x16x16x16", "nan_inf_raw", "ties_u16"])
def test_deterministic_and_independent_of_the_batch(ctx, name):
    """Two launches give the same bits, and a patch scored alone gives the bits it has inside its batch."""
    case = CASES[name]
    first = run_batch(ctx, case, 0.1)
    again = run_batch(ctx, case, 0.1)
    np.testing.assert_array_equal(first.view(np.uint64), again.view(np.uint64))
    for b in range(len(first)):
        alone = run_batch(ctx, tuple(a[b:b + 1] for a in case), 0.1)
        np.testing.assert_array_equal(alone.view(np.uint64), first[b:b + 1].view(np.uint64), err_msg=f"patch {b}")
    flipped = run_batch(ctx, tuple(a[::-1].copy() for a in case), 0.1)
    np.testing.assert_array_equal(flipped[::-1].view(np.uint64), first.view(np.uint64))


def test_a_bad_patch_leaves_its_neighbours_alone(ctx):
    """The clean patch of nan_inf_raw scores as it does in a batch of clean patches."""
    pred, raw, target, mask = CASES["nan_inf_raw"]
    rows = run_batch(ctx, (pred, raw, target, mask), 0.1)
    clean = run_batch(ctx, tuple(np.stack([a[0], a[0]]) for a in (pred, raw, target, mask)), 0.1)
    np.testing.assert_array_equal(rows[0].view(np.uint64), clean[0].view(np.uint64))
    np.testing.assert_array_equal(clean[1].view(np.uint64), clean[0].view(np.uint64))
    assert np.isnan(rows[1, nat.EVAL_MED]) and np.isnan(rows[1, nat.EVAL_THR]) and rows[1, 3] == 0
    assert np.isfinite(rows[2, nat.EVAL_MED]) and np.isinf(rows[2, 5])


def test_the_median_of_float32_data_is_fp64(ctx):
    rows = run_batch(ctx, CASES["halfway_median"], 0.1)
    for b in range(3):
        med = rows[b, nat.EVAL_MED]
        assert np.float64(np.float32(med)) != med, "the mean of two neighbouring float32 values is no float32"


@pytest.mark.parametrize("name", ["val_2x64x64x64", "u16_5x16x16x16", "f32_1x16x16x17", "mask_float", "mask_uint8",
                                  "nan_pred"])
def test_cuda_tensors_equal_their_host_copies(name):
    import torch
    case = CASES[name]
    for pct in (0.1, 50.0):
        host = metrics.evaluate_examples(*case, pct=pct)
        dev = metrics.evaluate_examples(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case), pct=pct)
        assert len(host) == len(dev)
        for h, d in zip(host, dev):
            assert tuple(h) == tuple(d) and all(P.same(d[k], h[k]) for k in h), (name, pct, h, d)
    # a non-contiguous view of a larger tensor
    wide = [torch.from_numpy(np.ascontiguousarray(np.concatenate([a, a], axis=3))).cuda() for a in case]
    half = case[0].shape[3]
    dev = metrics.evaluate_examples(*(w[..., :half] for w in wide), pct=0.1)
    for h, d in zip(metrics.evaluate_examples(*case, pct=0.1), dev):
        assert all(P.same(d[k], h[k]) for k in h)


def test_arguments_are_checked(ctx):
    pred, raw, target, mask = CASES["val_3x5x6x7"]
    assert metrics.evaluate_examples(pred[:0], raw[:0], target[:0], mask[:0]) == []
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred.astype(np.float64), raw, target, mask)
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred, raw.astype(np.int32), target, mask)
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred, raw, target[:1], mask)
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred[0], raw[0], target[0], mask[0])
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred, raw, target, mask.astype(np.int32))
    with pytest.raises(ValueError):
        metrics.evaluate_examples(pred, raw, target, mask, pct=101.0)
    n = pred[0].size
    d = [ctx.to_device(np.ascontiguousarray(a)) for a in (pred, raw, target, mask_bytes(mask))]
    try:
        def call(ranks, batch=3, nn=n, dts=(np.uint16, np.float32, np.uint16)):
            return ctx.evaluate_batch(d[0], dts[0], d[1], dts[1], d[2], dts[2], d[3], batch, nn, 6.0, ranks)
        good = ranks_of(n, 0.1)
        assert call(good).shape == (3, nat.EVAL_K)
        for bad in ([good[0], good[1], good[2], n], [good[1], good[0], good[2], good[3]], [0, 2, good[2], good[3]],
                    [good[0], good[1], good[3], good[2]]):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            call(good, batch=0)
        with pytest.raises(ValueError):
            call(good, nn=0)
        with pytest.raises(ValueError):
            call(good, dts=(np.float64, np.float32, np.uint16))
    finally:
        for b in d:
            b.free()


# ---- train.validate -----------------------------------------------------------------------------------------
class ZlibStub:
    """A host-only codec of the shape the reference passes (numcodecs' Blosc): ``encode(chunk) -> bytes``."""

    def encode(self, chunk):
        import zlib
        return zlib.compress(np.ascontiguousarray(chunk).tobytes(), 1)


def validate_setup():
    """The identity network on validate_inputs.validate_batches: predictions are x, so every expected value
    follows from the inputs without a convolution."""
    import torch
    from aind_exaspim_image_compression.machine_learning import losses, transforms

    class Identity(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.modes = []

        def forward(self, x):
            self.modes.append(self.training)
            return x

    batches = vi.validate_batches()
    tf = transforms.AsinhTransform(*vi.transform_args())
    crit = losses.SignalPreservingLoss()
    want_losses, want_rows, pred_counts = [], [], []
    for x, y, raw, mask in batches:
        d = x.astype(np.float64) - y.astype(np.float64)
        per_voxel = (1.0 + crit.fg_weight * mask.astype(np.float64)) * np.sqrt(d * d + crit.eps * crit.eps)
        want_losses.append(float(np.float32(per_voxel.mean())))          # the criterion returns an fp32 scalar
        for b in range(len(x)):
            p, t = tf.inverse(x[b, 0]), tf.inverse(y[b, 0])
            assert p.dtype == t.dtype == np.uint16
            pred_counts.append(p)
            want_rows.append(P.example(p, raw[b, 0], t, mask[b, 0]))
    return Identity(), batches, crit, tf, want_losses, want_rows, pred_counts


def check_validation(got, want, what):
    assert got["n"] == want["n"] and tuple(got["metrics"]) == P.METRICS, what
    for key in ("loss", "cratio", "score"):
        assert got[key] == want[key], f"{what} {key}: {got[key]!r} != {want[key]!r}"
    for key in P.METRICS:
        # both images of either MAE are uint16 here: every per-example value is the pyref's, so is their mean
        assert got["metrics"][key] == want["metrics"][key], f"{what} {key}"


@pytest.mark.parametrize("codec_kind", ["exac", "stub", "none"])
def test_validate(codec_kind):
    import torch
    from aind_exaspim_image_compression.machine_learning import train
    from aind_exaspim_image_compression.utils import img_util
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec

    net, batches, crit, tf, want_losses, want_rows, pred_counts = validate_setup()
    if codec_kind == "exac":
        codec = ExacCodec(2)
        ratios = [img_util.compute_cratio(p, ExacCodec(2)) for p in pred_counts]
    elif codec_kind == "stub":
        codec = ZlibStub()
        ratios = [round(p.nbytes / len(codec.encode(p)), 2) for p in pred_counts]
    else:
        codec = None
        ratios = [img_util.shuffled_entropy_cratio(p) for p in pred_counts]
    assert len(set(ratios)) > 1, "the median must have something to choose from"
    weights = {"fg_mae": 0.5, "bg_mae": 1.5, "top_pct_error": 0.25, "cratio": 2.0}
    for w in (None, weights):
        want = P.aggregate(want_losses, ratios, want_rows, w)
        as_tensors = [tuple(torch.from_numpy(a) for a in batch) for batch in batches]
        got = train.validate(net, as_tensors, crit, tf, codec=codec, checkpoint_weights=w)
        check_validation(got, want, f"{codec_kind} host tensors")
        on_device = [tuple(t.cuda() for t in batch) for batch in as_tensors]
        check_validation(train.validate(net, iter(on_device), crit, tf, codec=codec, checkpoint_weights=w), want,
                         f"{codec_kind} device tensors")
    assert net.training and net.modes and not any(net.modes), "eval mode during the pass, the old mode after it"
    # pct reaches the metrics
    got = train.validate(net, batches, crit, tf, codec=codec, pct=50.0)
    rows50 = [P.example(tf.inverse(x[b, 0]), raw[b, 0], tf.inverse(y[b, 0]), mask[b, 0], pct=50.0)
              for x, y, raw, mask in batches for b in range(len(x))]
    check_validation(got, P.aggregate(want_losses, ratios, rows50), f"{codec_kind} pct=50")


def test_validate_without_examples_and_with_a_bad_precision():
    from aind_exaspim_image_compression.machine_learning import train

    net, _, crit, tf, *_ = validate_setup()
    got = train.validate(net, [], crit, tf)
    assert got["score"] is None and np.isnan(got["loss"]) and np.isnan(got["cratio"]) and got["n"] == 0

    def never():
        raise AssertionError("the batches were touched")
        yield

    with pytest.raises(ValueError):
        train.validate(net, never(), crit, tf, precision="fp8")
