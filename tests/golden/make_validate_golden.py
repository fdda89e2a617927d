"""Generate tests/golden/validate_batch.npz by IMPORTING THE REFERENCE's evaluate_example and checkpoint_score
(machine_learning/metrics.py:384-455).

Run in the build container only (the reference does not exist on the GPU machine):

    PYTHONPATH=/path/to/reference/src python tests/golden/make_validate_golden.py

The fixture is data only: per case and percentile a (B, 6) float64 array of the reference's metric values in
validate_pyref.METRICS order, and two checkpoint scores per case; inputs are regenerated from seeds by
tests/validate_inputs.py.  The mask goes in as Trainer.compute_metrics hands it over (train.py:371): a float
mask as ``mask > 0.5``.
"""
import os
import sys
import warnings

import numpy as np

from aind_exaspim_image_compression.machine_learning import metrics as ref

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import validate_inputs as vi  # noqa: E402
from validate_pyref import METRICS  # noqa: E402

CRATIO = 3.21
CUSTOM_WEIGHTS = {"fg_mae": 0.5, "bg_mae": 1.5, "top_pct_error": 0.25, "cratio": 2.0}


def main():
    warnings.simplefilter("ignore")
    out = {}
    for name, (pred, raw, target, mask) in vi.all_cases().items():
        mask = mask > 0.5 if mask.dtype.kind == "f" else mask.astype(bool)
        for pct in vi.PCTS:
            with np.errstate(all="ignore"):
                rows = [ref.evaluate_example(pred[b], raw[b], target[b], mask[b], pct=pct) for b in range(len(pred))]
            assert all(tuple(r) == METRICS for r in rows)
            out[f"{name}/pct{pct:g}"] = np.array([[r[k] for k in METRICS] for r in rows], dtype=np.float64)
            if pct == 0.1:
                agg = {k: float(np.mean([r[k] for r in rows])) for k in METRICS}
                out[f"{name}/score"] = np.array([ref.checkpoint_score(agg, CRATIO),
                                                 ref.checkpoint_score(agg, CRATIO, CUSTOM_WEIGHTS)])
    out["inputs_sha256"] = np.array(vi.inputs_digest())
    np.savez_compressed(os.path.join(HERE, "validate_batch.npz"), **out)
    print(f"wrote {len(out)} arrays")


if __name__ == "__main__":
    main()
