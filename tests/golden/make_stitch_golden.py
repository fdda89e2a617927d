"""Generate tests/golden/stitch.npz by IMPORTING THE REFERENCE (the recipe of make_golden.py):

    PYTHONPATH=/root/reference/src python tests/golden/make_stitch_golden.py

The reference's ``predict`` is run on the CPU with a model that ignores its input, hands back seeded predictions
(``stitch_pyref.random_predictions``) and records what it was fed.  Stored per case: the uint16 volume ``predict``
returned, and for the first case the batches the model saw.  The fixture is data only: volumes and predictions are
regenerated from seeds by the test.  Only transforms without arcsinh / sinh are used, so nothing depends on the
host's SIMD math (see make_golden.py).
"""
import os
import sys

import numpy as np
import torch

from aind_exaspim_image_compression import inference as ref_inf
from aind_exaspim_image_compression.machine_learning import transforms as ref_tf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import stitch_pyref  # noqa: E402  (tests/stitch_pyref.py: the seeded predictions the test regenerates)

TRANSFORM_CFGS = {
    "anscombe_g8_rn5_o100": {"kind": "anscombe", "params": {"gain": 8.0, "read_noise": 5.0, "offset": 100.0}},
    "linear_35_1000_8": {"kind": "linear", "params": {"mn": 35.0, "mx": 1000.0, "clip": 8.0}},
}
CASES = {
    # name: (shape, patch, overlap, trim, batch, seed); "a": the last z patch is padded; "b": three cores deep
    "a": ((27, 24, 33), 16, 6, 2, 5, 21),
    "b": ((30, 17, 33), 16, 10, 1, 7, 22),
}


def case_volume(shape, seed):
    """uint16 counts of 16 distinct values (the recorded inputs then compress well)."""
    return (np.random.default_rng(seed).integers(0, 16, shape) * 70).astype(np.uint16)


class _Recorded(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.preds, self.k, self.seen = torch.from_numpy(preds)[:, None], 0, []

    def forward(self, x):
        n = x.shape[0]
        self.seen.append(x[:, 0].numpy().copy())
        self.k += n
        return self.preds[self.k - n:self.k]


if __name__ == "__main__":
    out = {}
    for cname, (shape, patch, overlap, trim, batch, seed) in CASES.items():
        vol = case_volume(shape, seed)
        n = ref_inf.count_patches(vol[None, None], patch, overlap)
        for tname, cfg in TRANSFORM_CFGS.items():
            model = _Recorded(stitch_pyref.random_predictions(n, patch, seed))
            res = ref_inf.predict(vol, model, ref_tf.build_transform(cfg), batch_size=batch, patch_size=patch,
                                  overlap=overlap, trim=trim, verbose=False)
            assert model.k == n and res.dtype == np.uint16 and res.shape == shape
            out[f"{cname}/{tname}/predict"] = res
            if cname == "a":
                out[f"{cname}/{tname}/inputs"] = np.concatenate(model.seen).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "stitch.npz"), **out)
    print("stitch.npz written:", os.path.getsize(os.path.join(HERE, "stitch.npz")), "bytes")
