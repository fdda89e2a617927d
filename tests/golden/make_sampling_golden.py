"""Generate tests/golden/sampling.npz by DRIVING THE REFERENCE's TrainDataset samplers
(machine_learning/data_handling.py:356-702) the way scripts/precompute.py:73-123 drives them.

Run in the build container only (the reference does not exist on the GPU machine):

    PYTHONPATH=/path/to/reference/src python tests/golden/make_sampling_golden.py

The fixture is data only: per (seed, split, index) of tests/sampling_inputs.py it stores the drawn brain, the
voxel and the bit-packed foreground mask; the inputs are regenerated from seeds.  The dataset's ``imgs`` /
``segmentations`` / ``skeletons`` dicts are filled with in-memory stand-ins.  Modules the reference imports at
module level and that are not installed (cloud clients, codecs, the closed bm4d wheel) get inert stubs in
``sys.modules`` -- none of them is called on the path driven here, except ``fastremap.unique``, whose stub is
``np.unique``.  The BM4D teacher is not recorded.
"""
import importlib
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sampling_inputs as si  # noqa: E402


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def import_with_stubs(name):
    stubbed = []
    while True:
        try:
            return importlib.import_module(name), stubbed
        except ModuleNotFoundError as e:
            if e.name is None or e.name.startswith("aind_exaspim_image_compression"):
                raise
            stub = _Stub(e.name)
            if e.name == "fastremap":
                stub.unique = np.unique
            sys.modules[e.name] = stub
            stubbed.append(e.name)


class _Read:
    def __init__(self, arr):
        self.arr = arr

    def read(self):
        return self

    def result(self):
        return self.arr


class Precomputed:
    """A (z, y, x) ndarray behind tensorstore's ``store[slices].read().result()``."""

    def __init__(self, arr):
        self.arr = arr

    def __getitem__(self, key):
        return _Read(self.arr[key])


def main():
    dh, stubbed = import_with_stubs("aind_exaspim_image_compression.machine_learning.data_handling")
    from aind_exaspim_image_compression.machine_learning.metrics import make_foreground_mask
    brains = si.brains()
    offsets = {k: b["offset"] for k, b in brains.items()}
    train = dh.TrainDataset(si.PATCH, offsets=offsets, **si.PARAMS)
    val = dh.ValidateDataset(si.PATCH, offsets=offsets)
    for name, b in brains.items():
        train.imgs[name] = b["image"][None, None]
        val.imgs[name] = b["val_image"][None, None]
        if b["labels"] is not None:
            train.segmentations[name] = Precomputed(b["labels"])
        if b["skeleton"] is not None:
            train.skeletons[name] = b["skeleton"]
    names = sorted(brains)
    out = {"inputs_sha256": np.array(si.inputs_digest())}
    for seed, split, index in si.GOLDEN_TASKS:
        states = np.random.SeedSequence([seed, {"train": 0, "val": 1}[split], index]).generate_state(2)
        random.seed(int(states[0]))
        np.random.seed(int(states[1]))
        if split == "train":           # TrainDataset._sample_counts without the teacher
            brain_id, voxel, raw, labels = train.sample_clean(train.read_counts)
            mask = train.foreground_mask(brain_id, voxel, raw, labels=labels)
        else:                          # precompute.py:116-123
            brain_id, voxel, raw, labels = train.sample_clean(val.read_counts)
            mask = train.annotation_mask(brain_id, voxel, labels=labels)
            if mask is None:
                mask = make_foreground_mask(raw)
        key = f"{seed}/{split}/{index}"
        out[f"brain/{key}"] = np.int64(names.index(brain_id))
        out[f"voxel/{key}"] = np.array([int(v) for v in voxel], dtype=np.int64)
        out[f"mask/{key}"] = np.packbits(np.asarray(mask, dtype=bool))
        out[f"rawsum/{key}"] = np.float64(np.asarray(raw, dtype=np.float64).sum())
    np.savez_compressed(os.path.join(HERE, "sampling.npz"), **out)
    print(f"wrote {len(out)} arrays; stubbed modules: {stubbed}")


if __name__ == "__main__":
    main()
