"""tests/validate_pyref.py against the reference: every value of tests/golden/validate_batch.npz, which holds what
the reference's evaluate_example and checkpoint_score return for the seeded inputs of tests/validate_inputs.py.
Values made of order statistics and counts are compared for equality, the two MAEs within
validate_pyref.mae_bound (a bound from the number format).  No GPU."""
import os

import numpy as np
import pytest

import validate_inputs as vi
import validate_pyref as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validate_batch.npz")
CRATIO = 3.21
CUSTOM_WEIGHTS = {"fg_mae": 0.5, "bg_mae": 1.5, "top_pct_error": 0.25, "cratio": 2.0}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return vi.all_cases()


def test_fixture_belongs_to_these_inputs(golden):
    assert str(golden["inputs_sha256"]) == vi.inputs_digest()
    assert len(vi.all_cases()) * (len(vi.PCTS) + 1) + 1 == len(golden)


def test_pyref_reproduces_the_reference(golden, cases):
    worst = 0.0
    for name, (pred, raw, target, mask) in cases.items():
        for pct in vi.PCTS:
            rows = P.examples(pred, raw, target, mask, pct)
            worst = max(worst, P.check_rows(rows, golden[f"{name}/pct{pct:g}"], rows, f"{name} pct={pct:g}",
                                          P.u16_pairs((pred, raw, target, mask))))
    print(f"\nlargest MAE error / bound: {worst:.3g}")


def test_aggregation_and_score(golden, cases):
    """Trainer.validate's aggregation: the mean of every metric over the examples, then checkpoint_score."""
    for name, (pred, raw, target, mask) in cases.items():
        want_rows = golden[f"{name}/pct0.1"]
        rows = [dict(zip(P.METRICS, r)) for r in want_rows]
        for weights, want in zip((None, CUSTOM_WEIGHTS), golden[f"{name}/score"]):
            agg = P.aggregate([0.5, 0.25], [CRATIO], rows, weights)
            assert P.same(agg["score"], want), name
            assert agg["loss"] == 0.375 and agg["cratio"] == CRATIO and agg["n"] == len(rows)
    empty = P.aggregate([], [], [])
    assert empty["score"] is None and np.isnan(empty["loss"]) and np.isnan(empty["cratio"])


def test_percentile_ranks_are_numpys():
    rng = np.random.default_rng(3)
    for n in (1, 2, 105, 210, 4096, 4352):
        x = rng.normal(size=n)
        s = np.sort(x)
        for pct in (0.0, 0.1, 1.0, 37.5, 50.0, 100.0):
            lo, hi = P.percentile_ranks(n, pct)
            got = np.percentile(x, 100.0 - pct)
            assert min(s[lo], s[hi]) <= got <= max(s[lo], s[hi])
            if lo == hi:
                assert got == s[lo]
