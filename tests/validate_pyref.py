"""The validation metrics in plain numpy, from their definitions (fp64 throughout, np.median, np.percentile):
the per-example dictionary of ``evaluate_example``, the intermediate values the device row carries, and the
aggregation of ``Trainer.validate``.  The yardstick of tests/test_validate_gpu.py; tests/test_validate_pyref.py
holds it against the reference's stored outputs."""
import warnings

import numpy as np

METRICS = ("fg_mae", "bg_mae", "top_pct_error", "top_pct_preservation", "mip_max_error", "false_bright_rate")
EXACT = ("top_pct_error", "top_pct_preservation", "mip_max_error", "false_bright_rate")
WEIGHTS = {"fg_mae": 1.0, "bg_mae": 0.2, "top_pct_error": 0.5, "cratio": 0.0}


def percentile_ranks(n, pct):
    """The two 0-based ranks np.percentile(x, 100 - pct) interpolates between (method "linear")."""
    virtual = (n - 1) * np.true_divide(100.0 - pct, 100.0)
    if virtual >= n - 1:
        return n - 1, n - 1
    return int(np.floor(virtual)), int(np.floor(virtual)) + 1


def _at_ranks(x, ranks):
    """Sorted x at ``ranks``; NaN when x holds a NaN (np.percentile of such data is NaN)."""
    if np.isnan(x).any():
        return [np.float64(np.nan)] * len(ranks)
    s = np.sort(x)
    return [s[r] for r in ranks]


def example(pred, raw, target, fg_mask, pct=0.1, k=6.0):
    """The metric dictionary of one example plus ``med``, ``mad``, ``thr``, the counts ``n_fg`` / ``n_bright``,
    the maxima, the rank values ``raw_lo`` / ``raw_hi`` / ``pred_lo`` / ``pred_hi``, the sums ``fg_sum`` /
    ``bg_sum`` and their term counts."""
    p64, r64, t64 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (pred, raw, target))
    fg = np.asarray(fg_mask)
    fg = (fg > 0.5 if fg.dtype.kind == "f" else fg.astype(bool)).reshape(-1)
    bg = ~fg
    n = p64.size
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        fg_sum = float(np.abs(p64 - r64)[fg].sum())
        bg_sum = float(np.abs(p64 - t64)[bg].sum())
        fg_mae = float(np.abs(p64 - r64)[fg].mean()) if fg.any() else 0.0
        bg_mae = float(np.abs(p64 - t64)[bg].mean()) if bg.any() else 0.0
        q = 100.0 - pct
        raw_top = float(np.percentile(r64, q))
        pred_top = float(np.percentile(p64, q))
        med = np.median(r64)
        mad = np.median(np.abs(r64 - med))
        thr = med + k * 1.4826 * (mad + 1e-6)
        n_bright = int(np.count_nonzero(p64[bg] > thr))
        mip = float(abs(np.max(pred) - np.max(raw)))      # the callers' dtypes: two uint16 maxima wrap
    ranks = percentile_ranks(n, pct)
    raw_lo, raw_hi = _at_ranks(r64, ranks)
    pred_lo, pred_hi = _at_ranks(p64, ranks)
    return {
        "fg_mae": fg_mae,
        "bg_mae": bg_mae,
        "top_pct_error": abs(pred_top - raw_top),
        "top_pct_preservation": pred_top / (raw_top + 1e-8),
        "mip_max_error": mip,
        "false_bright_rate": float(n_bright / bg.sum()) if bg.any() else 0.0,
        "med": float(med), "mad": float(mad), "thr": float(thr),
        "n_fg": int(fg.sum()), "n_bright": n_bright,
        "max_pred": float(np.max(p64)), "max_raw": float(np.max(r64)),
        "raw_lo": float(raw_lo), "raw_hi": float(raw_hi), "pred_lo": float(pred_lo), "pred_hi": float(pred_hi),
        "fg_sum": fg_sum, "bg_sum": bg_sum, "n": n,
    }


def examples(pred, raw, target, fg_mask, pct=0.1):
    return [example(pred[b], raw[b], target[b], fg_mask[b], pct) for b in range(len(pred))]


def checkpoint_score(metrics, cratio, weights=None):
    w = WEIGHTS if weights is None else weights
    return (w.get("fg_mae", 0.0) * metrics["fg_mae"] + w.get("bg_mae", 0.0) * metrics["bg_mae"]
            + w.get("top_pct_error", 0.0) * metrics["top_pct_error"] - w.get("cratio", 0.0) * cratio)


def aggregate(losses, cratios, rows, weights=None):
    """Trainer.validate's aggregation: mean loss, median ratio, mean of every metric, checkpoint score."""
    if not rows:
        return {"loss": float("nan"), "cratio": float("nan"), "score": None, "metrics": {}, "n": 0}
    loss = float(np.mean(losses))
    cratio = float(np.median(cratios))
    agg = {k: float(np.mean([row[k] for row in rows])) for k in METRICS}
    return {"loss": loss, "cratio": cratio, "score": checkpoint_score(agg, cratio, weights), "metrics": agg,
            "n": len(rows)}


def mae_bound(want, terms):
    """|got - want| allowed for a mean of ``terms`` non-negative fp64 terms summed in any order: each order is
    within (terms - 1) * 2^-53 relative of the true sum, numpy's and the kernel's alike."""
    return 2.0 * terms * 2.0 ** -53 * abs(want)


def same(got, want):
    """Equal values, NaN where ``want`` is NaN.  For floats that are neither NaN nor zero, equal values are equal
    bits."""
    got, want = float(got), float(want)
    return (np.isnan(got) and np.isnan(want)) or got == want


def check_rows(got_rows, want, pyref_rows, what, both_u16):
    """``got_rows``: metric dicts; ``want``: (B, 6) values in METRICS order; ``pyref_rows``: ``example`` rows, for the
    term counts; ``both_u16``: u16_pairs of the case.  Order-statistic and count metrics, MAEs of two uint16 images
    (integer sums below 2^53) and non-finite or zero MAEs must be the same; the other MAEs lie within mae_bound.
    Returns the largest error / bound ratio."""
    worst = 0.0
    for b, (got, ref) in enumerate(zip(got_rows, pyref_rows)):
        for j, key in enumerate(METRICS):
            w = want[b, j]
            if key in EXACT or both_u16[key]:
                assert same(got[key], w), f"{what} patch {b} {key}: {got[key]!r} != {w!r}"
                continue
            terms = ref["n_fg"] if key == "fg_mae" else ref["n"] - ref["n_fg"]
            if not np.isfinite(w) or terms == 0 or w == 0.0:
                assert same(got[key], w), f"{what} patch {b} {key}: {got[key]!r} != {w!r}"
                continue
            ratio = abs(got[key] - w) / mae_bound(w, terms)
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{what} patch {b} {key}: {got[key]!r} vs {w!r}, error / bound = {ratio:.3g}"
    return worst


def u16_pairs(case):
    pred, raw, target, _ = case
    return {"fg_mae": pred.dtype == raw.dtype == np.uint16, "bg_mae": pred.dtype == target.dtype == np.uint16}
