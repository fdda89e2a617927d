"""A serial restatement of the reference's patch sampler (machine_learning/data_handling.py:315-335, 356-409,
446-505, 518-702 and scripts/precompute.py:73-123), one task at a time over plain ndarray volumes, numpy and the
standard library only.  It seeds and consumes the GLOBAL generators (``random`` / ``np.random``) in the
reference's call order; masks come from tests/mask_pyref.py.  Where a box leaves the volume it is filled with 0
(image, after which no offset is subtracted there, and labels): the reference would fail there."""
import random

import numpy as np

import mask_pyref as mp

SEED_STREAMS = {"train": 0, "val": 1}


def seed_task(seed, split, index):
    states = np.random.SeedSequence([seed, SEED_STREAMS[split], index]).generate_state(2)
    random.seed(int(states[0]))
    np.random.seed(int(states[1]))


def cut(volume, center, patch_shape):
    """(patch, inside): the box img_util.get_slices centres at ``center``, 0 outside the volume."""
    start = [int(c) - d // 2 for c, d in zip(center, patch_shape)]
    out = np.zeros(patch_shape, volume.dtype)
    inside = np.zeros(patch_shape, bool)
    lo = [min(max(s, 0), n) for s, n in zip(start, volume.shape)]
    hi = [min(max(s + d, 0), n) for s, d, n in zip(start, patch_shape, volume.shape)]
    if all(b > a for a, b in zip(lo, hi)):
        src = tuple(slice(a, b) for a, b in zip(lo, hi))
        dst = tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, start))
        out[dst] = volume[src]
        inside[dst] = True
    return out, inside


def segmentation_score(labels_patch):
    _, cnts = np.unique(labels_patch, return_counts=True)
    return int(np.max(cnts[1:])) if len(cnts) > 1 else None


def skeleton_mask(points, start, patch_shape, dilate):
    start = np.asarray(start)
    pts = np.asarray(points)
    inside = np.all((pts >= start) & (pts < start + np.asarray(patch_shape)), axis=1)
    mask = np.zeros(tuple(patch_shape), bool)
    local = (pts[inside] - start).astype(int)
    if local.size:
        mask[local[:, 0], local[:, 1], local[:, 2]] = True
    return mp.dilate(mask, max(dilate, 0))


class RefSampler:
    """``brains``: id -> dict(image, val_image, labels, skeleton, offset) of (z, y, x) ndarrays (None = absent).
    ``gate(labels, raw) -> bool`` stands for patch_has_incoherent_segment with the sampler's coherence
    parameters."""

    def __init__(self, brains, patch_shape, boundary_buffer=5000, foreground_sampling_rate=0.5,
                 min_foreground_voxels=50, min_segmentation_volume=200, prefetch_foreground_sampling=16,
                 reject_incoherent_patches=False, max_resample_attempts=50, segmentation_dilate=0,
                 skeleton_radius=2, gate=None):
        self.brains, self.patch_shape = brains, tuple(patch_shape)
        self.boundary_buffer = boundary_buffer
        self.foreground_sampling_rate = foreground_sampling_rate
        self.min_foreground_voxels = min_foreground_voxels
        self.min_segmentation_volume = min_segmentation_volume
        self.prefetch_foreground_sampling = prefetch_foreground_sampling
        self.reject_incoherent_patches = reject_incoherent_patches
        self.max_resample_attempts = max_resample_attempts
        self.segmentation_dilate = segmentation_dilate
        self.skeleton_radius = skeleton_radius
        self.gate = gate

    # -- reads -----------------------------------------------------------------------------------------
    def read_patch(self, brain_id, center):
        return cut(self.brains[brain_id]["image"], center, self.patch_shape)[0]

    def read_counts(self, brain_id, center, split="train"):
        b = self.brains[brain_id]
        img = b["val_image"] if split == "val" and b["val_image"] is not None else b["image"]
        patch, inside = cut(img, center, self.patch_shape)
        raw = patch.astype(np.float32) - np.float32(b["offset"])
        return np.where(inside, raw, np.float32(0.0))

    def read_labels(self, brain_id, center):
        return cut(self.brains[brain_id]["labels"], center, self.patch_shape)[0]

    # -- draws -----------------------------------------------------------------------------------------
    def sample_brain(self):
        return random.sample(list(self.brains.keys()), 1)[0]

    def sample_interior_voxel(self, brain_id):
        voxel = []
        for s in self.brains[brain_id]["image"].shape:
            voxel.append(random.randint(self.boundary_buffer, s - self.boundary_buffer))
        return tuple(voxel)

    def sample_skeleton_voxel(self, brain_id):
        skel = self.brains[brain_id]["skeleton"]
        idx = random.randint(0, len(skel) - 1)
        radius = np.array(self.patch_shape) // 4
        shift = np.array([np.random.randint(-r, r + 1) for r in radius])
        return tuple(int(c) for c in skel[idx] + shift)

    def _search(self, brain_id, score, enough):
        best, best_voxel, cnt = 0, self.sample_interior_voxel(brain_id), 0
        while best < enough:
            voxels = [self.sample_interior_voxel(brain_id) for _ in range(self.prefetch_foreground_sampling)]
            for voxel in voxels:
                s = score(voxel)
                if s is not None and s > best:
                    best_voxel, best = voxel, s
            cnt += 1
            if cnt > 5:
                break
        return best_voxel

    def sample_segmentation_voxel(self, brain_id):
        return self._search(brain_id, lambda v: segmentation_score(self.read_labels(brain_id, v)),
                            self.min_segmentation_volume)

    def sample_bright_voxel(self, brain_id):
        return self._search(brain_id, lambda v: int(mp.fg_mask(self.read_patch(brain_id, v), 6.0, 1).sum()),
                            self.min_foreground_voxels)

    def sample_foreground_voxel(self, brain_id):
        b = self.brains[brain_id]
        if b["skeleton"] is not None and np.random.random() > 0.5:
            return self.sample_skeleton_voxel(brain_id)
        if b["labels"] is not None:
            return self.sample_segmentation_voxel(brain_id)
        return self.sample_bright_voxel(brain_id)

    def sample_voxel(self, brain_id):
        if random.random() < self.foreground_sampling_rate:
            return self.sample_foreground_voxel(brain_id)
        return self.sample_interior_voxel(brain_id)

    def sample_clean(self, split="train"):
        attempts = self.max_resample_attempts if self.reject_incoherent_patches else 1
        brain_id = voxel = raw = labels = None
        for _ in range(max(1, attempts)):
            brain_id = self.sample_brain()
            voxel = self.sample_voxel(brain_id)
            raw = self.read_counts(brain_id, voxel, split)
            labels = None
            if self.brains[brain_id]["labels"] is not None:
                labels = self.read_labels(brain_id, voxel)
                if self.reject_incoherent_patches and self.gate(labels, raw):
                    continue
            return brain_id, voxel, raw, labels
        return brain_id, voxel, raw, labels

    # -- masks -----------------------------------------------------------------------------------------
    def annotation_mask(self, brain_id, center, labels=None):
        b = self.brains[brain_id]
        mask = None
        if b["labels"] is not None:
            if labels is None:
                labels = self.read_labels(brain_id, center)
            mask = mp.dilate(np.asarray(labels) > 0, max(self.segmentation_dilate, 0))
        if b["skeleton"] is not None:
            start = [int(c) - d // 2 for c, d in zip(center, self.patch_shape)]
            skel = skeleton_mask(b["skeleton"], start, self.patch_shape, self.skeleton_radius)
            mask = skel if mask is None else (mask | skel)
        return mask

    def sample_counts(self, seed, split, index):
        """Task ``index``: (brain_id, voxel, raw, fg_mask) -- the teacher is the caller's."""
        seed_task(seed, split, index)
        brain_id, voxel, raw, labels = self.sample_clean(split)
        mask = self.annotation_mask(brain_id, voxel, labels=labels)
        if mask is None:
            mask = mp.fg_mask(raw, 6.0, 1)
        return brain_id, voxel, raw, mask
