"""Inputs of the sampler tests, regenerated from seeds (numpy only): the volumes, labels and skeletons of a few
small brains, the sampler parameters, and the (seed, split, index) triples tests/golden/sampling.npz records.
Shared by tests/golden/make_sampling_golden.py (which may import nothing of this repository's package) and the
tests."""
import hashlib

import numpy as np

SHAPE = (48, 64, 80)
PATCH = (16, 16, 16)
PARAMS = dict(boundary_buffer=12, foreground_sampling_rate=0.5, min_foreground_voxels=50,
              min_segmentation_volume=200, prefetch_foreground_sampling=4, segmentation_dilate=0,
              skeleton_radius=2, max_resample_attempts=50)
GOLDEN_TASKS = [(seed, split, index) for seed in (42, 7) for split in ("train", "val") for index in range(8)]


def _ball(shape, centre, radius):
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 <= radius * radius


def _tube(shape, z, y, radius):
    zz, yy, _ = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return (zz - z) ** 2 + (yy - y) ** 2 <= radius * radius


def _image(rng, signal):
    return np.clip(np.rint(rng.normal(100.0, 4.0, SHAPE) + signal), 0, 65535).astype(np.uint16)


def brains():
    """brain id -> dict(image, val_image, labels, skeleton, offset): (z, y, x) ndarrays, None where absent.
    ``annotated`` has labels (a long tube of > 200 voxels per patch, a small ball, a noisy block) and a skeleton
    along the tube, kept far enough inside that no drawn box leaves the volume; ``bare`` has neither."""
    rng = np.random.default_rng(20240611)
    tube, ball, block = _tube(SHAPE, 24, 30, 2.0), _ball(SHAPE, (30, 44, 24), 2.0), np.zeros(SHAPE, bool)
    block[14:20, 46:52, 50:58] = True
    signal = 400.0 * tube + 300.0 * ball + block * rng.choice([0.0, 900.0], SHAPE)
    labels = np.zeros(SHAPE, np.uint32)
    labels[tube], labels[ball], labels[block] = 7, 3, 9
    skeleton = np.array([[24, 30, x] for x in range(20, 61)], dtype=np.int64)
    blob = 500.0 * _ball(SHAPE, (20, 40, 50), 5.0) + 350.0 * _ball(SHAPE, (30, 20, 22), 3.0)
    return {
        "annotated": dict(image=_image(rng, signal), val_image=_image(rng, signal), labels=labels,
                          skeleton=skeleton, offset=37.0),
        "bare": dict(image=_image(rng, blob), val_image=_image(rng, blob), labels=None, skeleton=None, offset=0.0),
    }


def edge_brains():
    """One brain whose skeleton touches the volume's corner (boxes leave the array: the fill rule) and whose
    labels hold no 0 anywhere (the ``cnts[1:]`` rule drops the smallest label)."""
    rng = np.random.default_rng(5)
    labels = np.full(SHAPE, 2, np.int32)
    labels[:, :, 40:] = 5
    labels[20:28, 30:36, 10:30] = 11
    skeleton = np.array([[0, 0, 0], [1, 2, 3], [47, 63, 79], [24, 32, 40]], dtype=np.int64)
    return {"edge": dict(image=_image(rng, 200.0 * _ball(SHAPE, (24, 32, 40), 6.0)), val_image=None, labels=labels,
                         skeleton=skeleton, offset=12.5)}


def inputs_digest():
    h = hashlib.sha256()
    for name, b in sorted(brains().items()):
        for key in ("image", "val_image", "labels", "skeleton"):
            if b[key] is not None:
                h.update(np.ascontiguousarray(b[key]).tobytes())
        h.update(repr((name, b["offset"])).encode())
    h.update(repr((SHAPE, PATCH, sorted(PARAMS.items()), GOLDEN_TASKS)).encode())
    return h.hexdigest()
