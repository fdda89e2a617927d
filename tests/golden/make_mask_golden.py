"""Generate tests/golden/masks.npz by IMPORTING THE REFERENCE's mask builders and coherence gate
(machine_learning/metrics.py:32-303).

Run in the build container only (the reference does not exist on the GPU machine):

    PYTHONPATH=/path/to/reference/src python tests/golden/make_mask_golden.py

The fixture is data only: outputs are stored (masks bit-packed), inputs are regenerated from seeds
by tests/mask_inputs.py.  No stored autocorrelation or high-frequency fraction may lie within 1e-6
of a decision threshold, so the tests' 1e-10 tolerance can never flip a decision.
"""
import os
import sys

import numpy as np

from aind_exaspim_image_compression.machine_learning import metrics as ref

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mask_inputs as mi  # noqa: E402

MIN_AUTOCORR, MAX_HF = 0.4, 0.35


def away_from_thresholds(name, ac, hf):
    assert abs(ac - MIN_AUTOCORR) > 1e-6, (name, ac)
    assert abs(hf - MAX_HF) > 1e-6, (name, hf)


def main():
    out = {}
    for name, (raw, k, dilate) in mi.foreground_cases().items():
        out[f"fg/{name}"] = np.packbits(ref.make_foreground_mask(raw, k=k, dilate=dilate))
    for name, (labels, dilate) in mi.segmentation_cases().items():
        out[f"seg/{name}"] = np.packbits(ref.make_segmentation_mask(labels, dilate=dilate))
    for name, (pts, start, shape, dilate) in mi.skeleton_cases().items():
        out[f"skel/{name}"] = np.packbits(ref.make_skeleton_mask(pts, start, shape, dilate=dilate))
    for name, (raw, mask) in mi.score_cases().items():
        for lag in mi.LAGS:
            out[f"ac/{name}/lag{lag}"] = np.float64(ref.local_autocorr(raw, mask, lag=lag))
        out[f"hf/{name}"] = np.float64(ref.highfreq_energy_fraction(raw, mask))
        away_from_thresholds(name, float(out[f"ac/{name}/lag2"]), float(out[f"hf/{name}"]))
    for name, (labels, raw, min_vox) in mi.gate_cases().items():
        out[f"gate/{name}"] = np.bool_(ref.patch_has_incoherent_segment(labels, raw,
                                                                        min_segment_voxels=min_vox))
        r64 = np.asarray(raw, dtype=np.float64)
        for lid in np.unique(labels[labels > 0]):
            seg = labels == lid
            if seg.sum() >= min_vox:
                away_from_thresholds(f"{name}/{lid}", ref.local_autocorr(r64, seg),
                                     ref.highfreq_energy_fraction(r64, seg))
    out["inputs_sha256"] = np.array(mi.inputs_digest())
    np.savez_compressed(os.path.join(HERE, "masks.npz"), **out)
    print(f"wrote {len(out)} arrays; gate decisions:",
          {k[5:]: bool(v) for k, v in out.items() if k.startswith("gate/")})


if __name__ == "__main__":
    main()
