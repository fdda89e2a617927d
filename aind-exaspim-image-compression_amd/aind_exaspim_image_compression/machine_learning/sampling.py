"""Patch samplers over local stores, many tasks at a time.

The reference draws every training / validation patch with ``TrainDataset``'s samplers
(``machine_learning/data_handling.py:315-335, 356-409, 446-505, 518-702``) inside one process per patch
(``scripts/precompute.py:73-123``).  ``PatchSampler`` is those samplers over stores this package wrote:
the same parameters, the same method names for single draws, and a batched form in which the candidates
of all tasks of a round are read, scored and gated in a few device passes.

Every task owns its generators, seeded as ``scripts/precompute.py:73-88`` seeds the global ones
(``SeedSequence([seed, stream, index]).generate_state(2)`` into ``random.seed`` / ``np.random.seed``), and
consumes them in the reference's order, short circuits included.  A task is a small state machine (a
Python generator): it hands out requests -- "score the patches at these voxels of this brain" (``bright``:
``int(make_foreground_mask(patch).sum())`` of the un-subtracted uint16 patch; ``segmentation``:
``np.max(cnts[1:])`` of the label patch's sorted unique values) or "read the patch I drew and gate it"
(``patch``) -- and is resumed with the answers.  The driver advances all live tasks one round at a time and
groups their requests by kind and brain, so a round costs per group one ``read_patches(out="device")`` and
one ``foreground_counts`` or ``label_set`` call, and one ``incoherent_segments`` per brain for the round
of ``sample_clean``.  The result of task *i* is a function of (seed, split, *i*) and the sources only: it
does not depend on the batch, the grouping or the order of the tasks, and equals the task run alone through
the single-draw methods (``sample_task``).

A box that leaves the array is filled with 0, in the image (``StoredArray.read_patches``' rule: the fill
is written as it is, the offset is not subtracted from it) and in the labels.  The reference would fail
there (a short read makes ``bm4d`` and the cache's fixed shape reject the patch); with a
``boundary_buffer`` of at least half a patch it only happens to voxels drawn next to a skeleton point at
the volume's edge.
"""
import random

import numpy as np

from aind_exaspim_image_compression.machine_learning.data_handling import (
    CONFIG_KEYS, SEED_STREAMS, PatchCacheWriter)
from aind_exaspim_image_compression.machine_learning.transforms import build_transform

SCORE_ROUNDS = 6                # the searches stop after ``cnt > 5`` (data_handling.py:648-650, 699-701)


class BrainSource:
    """What the samplers read of one brain: ``image`` (a ``StoredArray``, (1, 1, z, y, x) uint16),
    ``labels`` (None, a (z, y, x) integer array-like that takes a basic slice -- ``np.memmap``, ``ndarray`` -- or
    a ``LabelArray``: a (1, 1, z, y, x) ``exac-labels`` store, read by regions on the device), ``skeleton`` (None, or (N, 3) integer zyx voxels), the brain's background ``offset``
    and ``val_image`` (None, or the store the ``val`` split reads its counts from)."""

    def __init__(self, image, labels=None, skeleton=None, offset=0.0, val_image=None):
        if image is None:
            raise ValueError("BrainSource: a brain needs an image")
        if len(image.shape) != 5:
            raise ValueError("BrainSource: the image is (1, 1, z, y, x)")
        if val_image is not None and tuple(val_image.shape) != tuple(image.shape):
            raise ValueError("BrainSource: the validation image must have the image's shape")
        if _is_label_store(labels):
            if tuple(labels.shape) != (1, 1) + tuple(image.shape[2:]):
                raise ValueError("BrainSource: a label store is (1, 1, z, y, x) of the image's extent")
        elif labels is not None:
            if len(labels.shape) != 3 or tuple(labels.shape) != tuple(image.shape[2:]):
                raise ValueError("BrainSource: labels are (z, y, x) of the image's extent")
            if np.dtype(labels.dtype).kind not in "iub":
                raise ValueError("BrainSource: labels must be integers")
        if skeleton is not None:
            skeleton = np.asarray(skeleton)
            if skeleton.ndim != 2 or skeleton.shape[1] != 3 or len(skeleton) == 0:
                raise ValueError("BrainSource: the skeleton is a non-empty (N, 3) array of zyx voxels")
            if not np.issubdtype(skeleton.dtype, np.integer):
                raise ValueError("BrainSource: skeleton points are integer voxels")
            if skeleton.min() < -2 ** 31 or skeleton.max() >= 2 ** 31:
                raise ValueError("BrainSource: skeleton points outside the int32 range")
        self.image, self.labels, self.skeleton = image, labels, skeleton
        self.offset, self.val_image = float(offset), val_image


def _is_label_store(labels):
    from aind_exaspim_image_compression.utils.store_labels import LabelArray
    return isinstance(labels, LabelArray)


class TaskRng:
    """The two generators of task ``index``: ``py`` stands for the ``random`` module and ``np`` for
    ``np.random`` after ``_seed_task(index)`` of ``scripts/precompute.py:73-88``."""

    def __init__(self, seed, stream, index):
        states = np.random.SeedSequence([int(seed), int(stream), int(index)]).generate_state(2)
        self.py = random.Random(int(states[0]))
        self.np = np.random.RandomState(int(states[1]))


class _GlobalRng:
    """The process-wide generators, as the reference uses them (seed None: not reproducible)."""
    py = random
    np = np.random


def patch_starts(voxels, patch_shape):
    """Box origins of patches centred at ``voxels`` (``img_util.get_slices``)."""
    return np.asarray(voxels, dtype=np.int64).reshape(-1, 3) - np.array([d // 2 for d in patch_shape])


def read_label_patches(labels, voxels, patch_shape):
    """(N, *patch_shape) label patches centred at ``voxels``; what lies outside the array is 0."""
    starts = patch_starts(voxels, patch_shape)
    out = np.zeros((len(starts),) + tuple(patch_shape), dtype=np.dtype(labels.dtype))
    for n, start in enumerate(starts):
        lo = np.clip(start, 0, labels.shape)
        hi = np.clip(start + np.array(patch_shape), 0, labels.shape)
        if np.all(hi > lo):
            src = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
            dst = tuple(slice(int(a - s), int(b - s)) for a, b, s in zip(lo, hi, start))
            out[n][dst] = np.asarray(labels[src])
    return out


def volume_from_label_list(counts, n_voxels):
    """``np.max(cnts[1:]) if len(cnts) > 1 else None`` of ``fastremap.unique(patch, return_counts=True)``
    (data_handling.py:637-645) from the patch's positive labels: ``counts`` are their voxel counts in
    ascending label order and the zeros are the ``n_voxels - sum(counts)`` voxels left.  When the patch
    holds no 0 the sorted list starts with the smallest label, so that label is the one dropped."""
    counts = np.asarray(counts, dtype=np.int64)
    zeros = int(n_voxels) - int(counts.sum())
    rest = counts if zeros > 0 else counts[1:]
    return int(rest.max()) if len(rest) else None


class DeviceScorer:
    """Serves the tasks' requests from the sources on the device: one read and one scoring call per
    group of a round (module docstring)."""

    def __init__(self, sampler):
        self.s = sampler
        self._points = {}                      # brain_id -> (device int32 zyx triples, N): one upload per brain

    def _image(self, brain_id, split):
        src = self.s.brains[brain_id]
        return src.val_image if split == "val" and src.val_image is not None else src.image

    def bright(self, brain_id, voxels):
        from aind_exaspim_image_compression import _native
        img = self.s.brains[brain_id].image
        patches = img.read_patches(voxels, self.s.patch_shape, out="device")
        try:
            ctx = _native.context(img.device)
            return [int(c) for c in ctx.foreground_counts(patches.buf, np.uint16, len(voxels),
                                                          self.s.patch_shape)]
        finally:
            patches.free()

    def segmentation(self, brain_id, voxels):
        from aind_exaspim_image_compression import _native
        from aind_exaspim_image_compression.machine_learning import metrics
        if _is_label_store(self.s.brains[brain_id].labels):
            return self._segmentation_of_store(brain_id, voxels)
        labels = self.labels(brain_id, voxels)
        n = int(np.prod(self.s.patch_shape))
        out = [None] * len(labels)
        # ids <= 0 of a signed type are one background to the device set but distinct values to np.unique
        host = [b for b in range(len(labels)) if labels.dtype.kind == "i" and labels[b].min() < 0]
        for b in host:
            cnts = np.unique(labels[b], return_counts=True)[1]
            out[b] = int(cnts[1:].max()) if len(cnts) > 1 else None
        rest = sorted(set(range(len(labels))) - set(host))
        if rest:
            lab = metrics._labels_dev(labels[rest])
            ctx = _native.context(self.s.brains[brain_id].image.device)
            with ctx.to_device(lab) as d_labels:
                lists = metrics._label_lists(ctx, d_labels, lab, len(rest), self.s.patch_shape)
            for b, (_, counts) in zip(rest, lists):
                out[b] = volume_from_label_list(counts, n)
        return out

    def _segmentation_of_store(self, brain_id, voxels):
        """``segmentation`` for a ``LabelArray`` brain: the candidates' label patches go from the coded chunks to the
        device set without a visit to the host (only a patch the set cannot hold is downloaded and counted there)."""
        from aind_exaspim_image_compression import _native
        store = self.s.brains[brain_id].labels
        n = int(np.prod(self.s.patch_shape))
        patches = store.read_patches(voxels, self.s.patch_shape, out="device")
        try:
            ctx = _native.context(store.device)
            keys, counts, held, status = ctx.label_set(patches.buf, store.dtype, len(voxels), self.s.patch_shape)
            host = patches.download() if status.any() else None
        finally:
            patches.free()
        out = []
        for b in range(len(voxels)):
            if status[b]:
                lb = host[b]
                c = np.unique(lb[lb > 0], return_counts=True)[1]
            else:
                c = counts[b, :held[b]][np.argsort(keys[b, :held[b]], kind="stable")]
            out.append(volume_from_label_list(c, n))
        return out

    def raw_counts(self, brain_id, voxels, split):
        return self._image(brain_id, split).read_patches(voxels, self.s.patch_shape, dtype=np.float32,
                                                         offset=self.s.brains[brain_id].offset)

    def labels(self, brain_id, voxels):
        labels = self.s.brains[brain_id].labels
        if _is_label_store(labels):
            return labels.read_patches(voxels, self.s.patch_shape)
        return read_label_patches(labels, voxels, self.s.patch_shape)

    def incoherent(self, labels, raws):
        from aind_exaspim_image_compression.machine_learning import metrics
        s = self.s
        return metrics.incoherent_segments(labels, raws, s.coherence_min_autocorr, s.coherence_max_highfreq_frac,
                                           s.coherence_min_segment_voxels, s.coherence_smooth_sigma,
                                           s.coherence_lag)

    def annotation_masks(self, brain_id, voxels, labels):
        from aind_exaspim_image_compression import _native
        from aind_exaspim_image_compression.machine_learning import metrics
        src = self.s.brains[brain_id]
        ctx = _native.context(src.image.device)
        shape = (len(voxels),) + self.s.patch_shape
        d_labels = d_mask = None
        try:
            lab = None
            if labels is not None and _is_label_store(src.labels):
                # the patches at these voxels, from the coded chunks to the kernel (``labels`` holds the same values)
                lab = src.labels.read_patches(voxels, self.s.patch_shape, out="device")
                d_labels = lab.buf
            elif labels is not None:
                lab = metrics._labels_dev(np.asarray(labels))
                d_labels = ctx.to_device(lab)
            pts, npts = (None, 0)
            if src.skeleton is not None:
                if brain_id not in self._points:
                    p = np.ascontiguousarray(src.skeleton, dtype=np.int32)
                    self._points[brain_id] = (ctx.to_device(p), len(p))
                pts, npts = self._points[brain_id]
            d_mask = ctx.alloc(int(np.prod(shape)))
            ctx.annotation_masks(d_labels, lab.dtype if lab is not None else np.uint8,
                                 max(int(self.s.segmentation_dilate), 0), pts, npts,
                                 patch_starts(voxels, self.s.patch_shape), max(int(self.s.skeleton_radius), 0),
                                 self.s.patch_shape, d_mask)
            return d_mask.download(shape, np.uint8).view(bool)
        finally:
            for d in (d_labels, d_mask):
                if d is not None:
                    d.free()

    def foreground_masks(self, raws):
        from aind_exaspim_image_compression.machine_learning import metrics
        return metrics.foreground_masks(raws)

    def teacher(self, raws):
        from aind_exaspim_image_compression.bm4d import denoise_patches
        return denoise_patches(raws, sigma=float(self.s.sigma_bm4d), max_count=float(self.s.transform.max_count))

    def close(self):
        for buf, _ in self._points.values():
            buf.free()
        self._points = {}


class PatchSampler:
    """The reference ``TrainDataset``'s samplers (data_handling.py:99-122 for the parameters, their names
    and defaults) over ``brains``: a dict brain id -> ``BrainSource``.  ``scorer`` replaces the device
    (``DeviceScorer``) by another object with its methods."""

    def __init__(self, brains, patch_shape, boundary_buffer=5000, foreground_sampling_rate=0.5,
                 min_foreground_voxels=50, min_segmentation_volume=200, prefetch_foreground_sampling=16,
                 reject_incoherent_patches=False, coherence_min_autocorr=0.4, coherence_max_highfreq_frac=0.35,
                 coherence_min_segment_voxels=50, coherence_smooth_sigma=1.0, coherence_lag=2,
                 max_resample_attempts=50, segmentation_dilate=0, sigma_bm4d=16, skeleton_radius=2,
                 transform=None, scorer=None):
        self.patch_shape = tuple(int(d) for d in patch_shape)
        if len(self.patch_shape) != 3 or min(self.patch_shape) < 1:
            raise ValueError("PatchSampler: patch_shape is three positive sizes")
        self.brains = dict(brains)
        if not self.brains:
            raise ValueError("PatchSampler: no brains")
        for brain_id, src in self.brains.items():
            if not isinstance(src, BrainSource):
                raise ValueError(f"PatchSampler: brain {brain_id!r} is not a BrainSource")
            if any(s - boundary_buffer < boundary_buffer for s in src.image.shape[2:]):
                raise ValueError(f"PatchSampler: boundary_buffer {boundary_buffer} leaves no interior in brain "
                                 f"{brain_id!r} of shape {tuple(src.image.shape[2:])}")
        if prefetch_foreground_sampling < 1:
            raise ValueError("PatchSampler: prefetch_foreground_sampling must be >= 1")
        self.boundary_buffer = int(boundary_buffer)
        self.foreground_sampling_rate = foreground_sampling_rate
        self.min_foreground_voxels = min_foreground_voxels
        self.min_segmentation_volume = min_segmentation_volume
        self.prefetch_foreground_sampling = int(prefetch_foreground_sampling)
        self.reject_incoherent_patches = bool(reject_incoherent_patches)
        self.coherence_min_autocorr = coherence_min_autocorr
        self.coherence_max_highfreq_frac = coherence_max_highfreq_frac
        self.coherence_min_segment_voxels = coherence_min_segment_voxels
        self.coherence_smooth_sigma = coherence_smooth_sigma
        self.coherence_lag = coherence_lag
        self.max_resample_attempts = max_resample_attempts
        self.segmentation_dilate = segmentation_dilate
        self.sigma_bm4d = sigma_bm4d
        self.skeleton_radius = skeleton_radius
        self.transform = transform or build_transform({"kind": "asinh"})
        self.scorer = scorer if scorer is not None else DeviceScorer(self)

    # ---- the state machine: generators that yield (kind, brain_id, voxels) and are sent the answers ------
    def _interior(self, brain_id, rng):
        bb = self.boundary_buffer
        return tuple(rng.py.randint(bb, s - bb) for s in self.brains[brain_id].image.shape[2:])

    def _search(self, kind, brain_id, rng, enough):
        """sample_bright_voxel / sample_segmentation_voxel: rounds of ``prefetch_foreground_sampling``
        candidates; the first strictly larger score wins, in submission order; at most 6 rounds, and a
        search that has found ``enough`` draws no further round."""
        best, best_voxel = 0, self._interior(brain_id, rng)
        for _ in range(SCORE_ROUNDS):
            if not best < enough:
                break
            voxels = [self._interior(brain_id, rng) for _ in range(self.prefetch_foreground_sampling)]
            scores = yield (kind, brain_id, voxels)
            for voxel, score in zip(voxels, scores):
                if score is not None and score > best:
                    best, best_voxel = score, voxel
        return best_voxel

    def _skeleton_voxel(self, brain_id, rng):
        skel = self.brains[brain_id].skeleton
        idx = rng.py.randint(0, len(skel) - 1)
        shift = np.array([rng.np.randint(-r, r + 1) for r in np.array(self.patch_shape) // 4])
        return tuple(int(c) for c in skel[idx] + shift)

    def _foreground(self, brain_id, rng):
        src = self.brains[brain_id]
        if src.skeleton is not None and rng.np.random_sample() > 0.5:   # drawn only for brains with a skeleton
            return self._skeleton_voxel(brain_id, rng)
        if src.labels is not None:
            return (yield from self._search("segmentation", brain_id, rng, self.min_segmentation_volume))
        return (yield from self._search("bright", brain_id, rng, self.min_foreground_voxels))

    def _voxel(self, brain_id, rng):
        if rng.py.random() < self.foreground_sampling_rate:
            return (yield from self._foreground(brain_id, rng))
        return self._interior(brain_id, rng)

    def _brain(self, rng):
        return rng.py.sample(list(self.brains), 1)[0]

    def _clean(self, rng):
        """sample_clean: (brain_id, voxel); the driver keeps what it read for the last ``patch`` request."""
        attempts = self.max_resample_attempts if self.reject_incoherent_patches else 1
        brain_id = voxel = None
        for _ in range(max(1, attempts)):
            brain_id = self._brain(rng)
            voxel = yield from self._voxel(brain_id, rng)
            incoherent = yield ("patch", brain_id, [voxel])
            if not incoherent[0]:
                break
        return brain_id, voxel

    # ---- the driver ----------------------------------------------------------------------------------
    def _advance(self, tasks, split, read_counts=None):
        """Run the generators ``tasks`` to their ends, a round at a time: ``(results, kept)`` with
        ``kept[i]`` the (raw, labels) read for task i's last ``patch`` request."""
        n = len(tasks)
        results, kept, pending = [None] * n, [None] * n, {}

        def step(i, answer):
            try:
                pending[i] = tasks[i].send(answer)
            except StopIteration as stop:
                pending.pop(i, None)
                results[i] = stop.value

        for i in range(n):
            step(i, None)
        while pending:
            groups = {}
            for i, (kind, brain_id, _) in pending.items():
                groups.setdefault((kind, brain_id), []).append(i)
            answers = {}
            for (kind, brain_id), members in groups.items():
                voxels = [v for i in members for v in pending[i][2]]
                if kind == "patch":
                    scores = self._read_and_gate(brain_id, voxels, split, read_counts, members, kept)
                else:
                    scores = getattr(self.scorer, kind)(brain_id, voxels)
                at = 0
                for i in members:
                    k = len(pending[i][2])
                    answers[i] = scores[at:at + k]
                    at += k
            for i in list(pending):
                step(i, answers[i])
        return results, kept

    def _read_and_gate(self, brain_id, voxels, split, read_counts, members, kept):
        if read_counts is None:
            raws = self.scorer.raw_counts(brain_id, voxels, split)
        else:
            raws = np.stack([np.asarray(read_counts(brain_id, v), dtype=np.float32) for v in voxels])
        labels, flags = None, [False] * len(voxels)
        if self.brains[brain_id].labels is not None:
            labels = self.scorer.labels(brain_id, voxels)
            if self.reject_incoherent_patches:
                flags = [bool(f) for f in self.scorer.incoherent(labels, raws)]
        for j, i in enumerate(members):
            kept[i] = (raws[j], None if labels is None else labels[j])
        return flags

    def _run(self, gen, split="train", read_counts=None):
        results, kept = self._advance([gen], split, read_counts)
        return results[0], kept[0]

    def _masks(self, brain_ids, voxels, raws, labels):
        """annotation_mask of every draw, one call per annotated brain; make_foreground_mask(raw) for the
        draws of brains with neither annotation, in one call."""
        masks = np.zeros(raws.shape, dtype=bool)
        bare = []
        by_brain = {}
        for n, brain_id in enumerate(brain_ids):
            src = self.brains[brain_id]
            if src.labels is None and src.skeleton is None:
                bare.append(n)
            else:
                by_brain.setdefault(brain_id, []).append(n)
        for brain_id, members in by_brain.items():
            lab = None
            if self.brains[brain_id].labels is not None:
                lab = np.stack([labels[n] for n in members])
            masks[members] = self.scorer.annotation_masks(brain_id, [voxels[n] for n in members], lab)
        if bare:
            masks[bare] = self.scorer.foreground_masks(np.ascontiguousarray(raws[bare]))
        return masks

    def _rng(self, seed, split, index):
        if split not in SEED_STREAMS:
            raise ValueError(f"split must be one of {sorted(SEED_STREAMS)}")
        return _GlobalRng if seed is None else TaskRng(seed, SEED_STREAMS[split], index)

    def draw(self, task_indices, seed, split="train", teacher=True):
        """The tasks ``task_indices`` of ``scripts/precompute.py``'s ``_sample_counts``, advanced together:
        ``(brain_ids, voxels (N, 3), raw, teacher, fg_mask)`` in the order given.  ``val``
        (precompute.py:116-123): the draw and the mask come from the training sources, the counts from the
        validation image.  ``teacher=False`` leaves the BM4D teacher out (None)."""
        task_indices = [int(i) for i in task_indices]
        shape = (len(task_indices),) + self.patch_shape
        if not task_indices:
            return ([], np.zeros((0, 3), np.int64), np.zeros(shape, np.float32),
                    np.zeros(shape, np.float32) if teacher else None, np.zeros(shape, bool))
        tasks = [self._clean(self._rng(seed, split, i)) for i in task_indices]
        results, kept = self._advance(tasks, split)
        brain_ids = [r[0] for r in results]
        voxels = [r[1] for r in results]
        raws = np.stack([k[0] for k in kept]).astype(np.float32, copy=False)
        masks = self._masks(brain_ids, voxels, raws, [k[1] for k in kept])
        return (brain_ids, np.array(voxels, dtype=np.int64).reshape(-1, 3), raws,
                self.scorer.teacher(raws) if teacher else None, masks)

    def sample_counts(self, task_indices, seed, split="train", batch_tasks=64, teacher=True):
        """``draw`` in batches of ``batch_tasks`` tasks; the result does not depend on ``batch_tasks``."""
        task_indices = list(task_indices)
        if batch_tasks < 1:
            raise ValueError("batch_tasks must be >= 1")
        parts = [self.draw(task_indices[a:a + batch_tasks], seed, split, teacher)
                 for a in range(0, len(task_indices), batch_tasks)] or [self.draw([], seed, split, teacher)]
        return ([b for p in parts for b in p[0]], np.concatenate([p[1] for p in parts]),
                np.concatenate([p[2] for p in parts]),
                np.concatenate([p[3] for p in parts]) if teacher else None, np.concatenate([p[4] for p in parts]))

    def sample_task(self, index, seed, split="train", teacher=True):
        """One task alone, through the single-draw methods: ``(brain_id, voxel, raw, teacher, fg_mask)``."""
        rng = self._rng(seed, split, index)
        brain_id, voxel, raw, labels = self.sample_clean(rng=rng, split=split)
        mask = self.foreground_mask(brain_id, voxel, raw, labels=labels)
        return brain_id, voxel, raw, self.scorer.teacher(raw[None])[0] if teacher else None, mask

    # ---- single draws, with the reference's names (rng None: the process-wide generators) ---------------
    def sample_brain(self, rng=None):
        return self._brain(rng or _GlobalRng)

    def sample_interior_voxel(self, brain_id, rng=None):
        return self._interior(brain_id, rng or _GlobalRng)

    def sample_skeleton_voxel(self, brain_id, rng=None):
        return self._skeleton_voxel(brain_id, rng or _GlobalRng)

    def sample_voxel(self, brain_id, rng=None):
        return self._run(self._voxel(brain_id, rng or _GlobalRng))[0]

    def sample_foreground_voxel(self, brain_id, rng=None):
        return self._run(self._foreground(brain_id, rng or _GlobalRng))[0]

    def sample_segmentation_voxel(self, brain_id, rng=None):
        return self._run(self._search("segmentation", brain_id, rng or _GlobalRng,
                                      self.min_segmentation_volume))[0]

    def sample_bright_voxel(self, brain_id, rng=None):
        return self._run(self._search("bright", brain_id, rng or _GlobalRng, self.min_foreground_voxels))[0]

    def read_counts(self, brain_id, center, split="train"):
        """The float32 patch at ``center`` minus the brain's offset (0 outside the array)."""
        return self.scorer.raw_counts(brain_id, [center], split)[0]

    def sample_clean(self, read_counts=None, rng=None, split="train"):
        """``(brain_id, voxel, raw, labels)``: draws until the coherence gate passes a patch, or returns
        the last draw once ``max_resample_attempts`` are spent (data_handling.py:356-409).  ``read_counts``:
        None for ``self.read_counts`` of ``split``, or a callable (brain_id, voxel) -> counts."""
        (brain_id, voxel), (raw, labels) = self._run(self._clean(rng or _GlobalRng), split, read_counts)
        return brain_id, voxel, raw, labels

    def skeleton_mask(self, brain_id, center):
        """The brain's skeleton points inside the patch, dilated ``skeleton_radius`` times."""
        if self.brains[brain_id].skeleton is None:
            raise ValueError(f"brain {brain_id!r} has no skeleton")
        return self.scorer.annotation_masks(brain_id, [center], None)[0]

    def annotation_mask(self, brain_id, center, labels=None):
        """Segmentation mask | skeleton mask of the patch, or None for a brain with neither
        (data_handling.py:446-481)."""
        src = self.brains[brain_id]
        if src.labels is None and src.skeleton is None:
            return None
        if src.labels is not None and labels is None:
            labels = self.scorer.labels(brain_id, [center])[0]
        lab = None if src.labels is None else np.asarray(labels)[None]
        return self.scorer.annotation_masks(brain_id, [center], lab)[0]

    def foreground_mask(self, brain_id, center, raw, labels=None):
        mask = self.annotation_mask(brain_id, center, labels=labels)
        return self.scorer.foreground_masks(np.asarray(raw, dtype=np.float32)[None])[0] if mask is None else mask

    def close(self):
        """Release what the scorer keeps on the device (the brains' skeleton points)."""
        if hasattr(self.scorer, "close"):
            self.scorer.close()

    def config(self):
        """The ``CONFIG_KEYS`` entries the sampler knows (the writer adds its own)."""
        return {"foreground_sampling_rate": self.foreground_sampling_rate,
                "min_foreground_voxels": self.min_foreground_voxels,
                "min_segmentation_volume": self.min_segmentation_volume,
                "skeleton_radius": self.skeleton_radius, "segmentation_dilate": self.segmentation_dilate,
                "reject_incoherent_patches": self.reject_incoherent_patches,
                "coherence_min_autocorr": self.coherence_min_autocorr,
                "coherence_max_highfreq_frac": self.coherence_max_highfreq_frac,
                "coherence_min_segment_voxels": self.coherence_min_segment_voxels,
                "coherence_smooth_sigma": self.coherence_smooth_sigma, "coherence_lag": self.coherence_lag,
                "max_resample_attempts": self.max_resample_attempts}


def precompute_cache(cache_dir, sampler, n_patches, split="train", seed=None, batch_tasks=64, config=None):
    """The reference's ``precompute()`` (scripts/precompute.py:126-240) from local stores: tasks
    0 .. n_patches - 1 of ``split`` drawn ``batch_tasks`` at a time and written through
    ``PatchCacheWriter`` (which computes the teacher of each batch): ``raw.npy`` / ``teacher.npy`` /
    ``fg.npy``, ``config.json`` with every key the sampler knows plus ``config`` (keys outside
    ``CONFIG_KEYS`` raise), ``transform.json`` last."""
    cfg = dict(config or {})
    unknown = set(cfg) - set(CONFIG_KEYS)
    if unknown:
        raise ValueError(f"unknown config keys: {sorted(unknown)}")
    cfg.update(sampler.config())
    if batch_tasks < 1:
        raise ValueError("batch_tasks must be >= 1")
    with PatchCacheWriter(cache_dir, n_patches, patch_shape=sampler.patch_shape,
                          transform_cfg=sampler.transform.cfg, sigma_bm4d=sampler.sigma_bm4d, split=split,
                          seed=seed, config=cfg, batch_patches=batch_tasks) as writer:
        for a in range(0, int(n_patches), int(batch_tasks)):
            _, _, raw, _, fg = sampler.draw(range(a, min(a + int(batch_tasks), int(n_patches))), seed, split,
                                            teacher=False)
            writer.write(raw, fg)
    return writer.cache_dir
