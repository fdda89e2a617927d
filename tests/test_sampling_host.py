"""machine_learning/sampling.py without a GPU: the per-task generators, and the tasks' state machine driven with
a numpy scorer in place of the device, against the serial restatement (tests/sampling_pyref.py) and against what
the reference's TrainDataset drew (tests/golden/sampling.npz).  Every comparison is exact."""
import os
import random

import numpy as np
import pytest

import mask_pyref as mp
import sampling_inputs as si
import sampling_pyref as ref
from aind_exaspim_image_compression.machine_learning import sampling

HERE = os.path.dirname(os.path.abspath(__file__))


def fake_gate(labels, raw):
    """A stand-in for the coherence gate that rejects about a third of the annotated draws."""
    return int(np.asarray(raw, dtype=np.float64).sum()) % 3 == 0


class NumpyScorer:
    """sampling.DeviceScorer's methods over ndarray volumes, numpy only; counts what it is asked."""

    def __init__(self, brains, patch_shape, gate=fake_gate, segmentation_dilate=0, skeleton_radius=2):
        self.r = ref.RefSampler(brains, patch_shape, segmentation_dilate=segmentation_dilate,
                                skeleton_radius=skeleton_radius)
        self.gate = gate
        self.calls = {"bright": 0, "segmentation": 0, "patch": 0}

    def bright(self, brain_id, voxels):
        self.calls["bright"] += 1
        return [int(mp.fg_mask(self.r.read_patch(brain_id, v), 6.0, 1).sum()) for v in voxels]

    def segmentation(self, brain_id, voxels):
        self.calls["segmentation"] += 1
        return [ref.segmentation_score(self.r.read_labels(brain_id, v)) for v in voxels]

    def raw_counts(self, brain_id, voxels, split):
        self.calls["patch"] += len(voxels)
        return np.stack([self.r.read_counts(brain_id, v, split) for v in voxels])

    def labels(self, brain_id, voxels):
        return np.stack([self.r.read_labels(brain_id, v) for v in voxels])

    def incoherent(self, labels, raws):
        return [self.gate(lab, raw) for lab, raw in zip(labels, raws)]

    def annotation_masks(self, brain_id, voxels, labels):
        return np.stack([self.r.annotation_mask(brain_id, v, labels=None if labels is None else labels[n])
                         for n, v in enumerate(voxels)])

    def foreground_masks(self, raws):
        return np.stack([mp.fg_mask(r, 6.0, 1) for r in raws])

    def teacher(self, raws):
        return np.zeros_like(raws)


def sources(brains):
    return {name: sampling.BrainSource(b["image"][None, None], labels=b["labels"], skeleton=b["skeleton"],
                                       offset=b["offset"],
                                       val_image=None if b["val_image"] is None else b["val_image"][None, None])
            for name, b in brains.items()}


def make(brains, gate=fake_gate, **params):
    """(sampler on a numpy scorer, the serial reference) with the same parameters."""
    p = dict(si.PARAMS)
    p.update(params)
    scorer = NumpyScorer(brains, si.PATCH, gate, p["segmentation_dilate"], p["skeleton_radius"])
    return (sampling.PatchSampler(sources(brains), si.PATCH, scorer=scorer, **p),
            ref.RefSampler(brains, si.PATCH, gate=gate, **p))


@pytest.fixture(scope="module")
def world():
    brains = si.brains()
    brains.update(si.edge_brains())
    return brains


def assert_same(got, want_rows):
    brain_ids, voxels, raw, _, masks = got
    assert len(brain_ids) == len(want_rows)
    for n, (b, v, r, m) in enumerate(want_rows):
        assert brain_ids[n] == b, n
        assert tuple(voxels[n]) == tuple(v), n
        assert raw[n].dtype == np.float32 and np.array_equal(raw[n], r), n
        assert np.array_equal(masks[n], m), n


def test_task_generators_equal_the_reference_global_seeding():
    for seed, split, index in [(42, "train", 0), (42, "val", 0), (7, "train", 123456), (0, "val", 3)]:
        rng = sampling.TaskRng(seed, sampling.SEED_STREAMS[split], index)
        ref.seed_task(seed, split, index)
        for _ in range(5):
            assert rng.py.random() == random.random()
            assert rng.py.randint(12, 5000) == random.randint(12, 5000)
            assert rng.py.sample(list("abcdefg"), 1) == random.sample(list("abcdefg"), 1)
            assert rng.np.random_sample() == np.random.random()
            assert rng.np.randint(-4, 5) == np.random.randint(-4, 5)
        assert rng.py.getstate() == random.getstate()


@pytest.mark.parametrize("split", ["train", "val"])
def test_state_machine_equals_the_serial_reference(world, split):
    sampler, serial = make(world, reject_incoherent_patches=True, max_resample_attempts=3)
    pairs = [(seed, index) for seed in (1, 42, 2024) for index in range(20)]        # 60 pairs per split
    kinds = set()
    for seed in (1, 42, 2024):
        idx = [i for s, i in pairs if s == seed]
        want = [serial.sample_counts(seed, split, i) for i in idx]
        assert_same(sampler.sample_counts(idx, seed, split, teacher=False), want)
        kinds |= {w[0] for w in want}
    assert kinds == set(world)                      # every brain was drawn, the one at the edge included
    assert all(sampler.scorer.calls[k] > 0 for k in ("bright", "segmentation", "patch"))


def test_state_machine_equals_what_the_reference_drew():
    golden = np.load(os.path.join(HERE, "golden", "sampling.npz"))
    assert str(golden["inputs_sha256"]) == si.inputs_digest(), "regenerate tests/golden/sampling.npz"
    brains = si.brains()
    names = sorted(brains)
    sampler, serial = make(brains)
    for seed, split, index in si.GOLDEN_TASKS:
        key = f"{seed}/{split}/{index}"
        b, v, raw, _, mask = sampler.sample_counts([index], seed, split, teacher=False)
        assert b[0] == names[int(golden[f"brain/{key}"])], key
        assert tuple(v[0]) == tuple(golden[f"voxel/{key}"]), key
        assert np.array_equal(np.packbits(mask[0]), golden[f"mask/{key}"]), key
        assert float(raw[0].astype(np.float64).sum()) == float(golden[f"rawsum/{key}"]), key
        sb, sv, _, sm = serial.sample_counts(seed, split, index)                    # the restatement too
        assert (sb, tuple(sv)) == (b[0], tuple(v[0])) and np.array_equal(sm, mask[0]), key


def test_result_does_not_depend_on_the_batch_or_the_task_order(world):
    sampler, serial = make(world, reject_incoherent_patches=True, max_resample_attempts=4)
    idx = list(range(17))
    want = [serial.sample_counts(9, "train", i) for i in idx]
    for batch_tasks in (1, 3, 64):
        assert_same(sampler.sample_counts(idx, 9, "train", batch_tasks=batch_tasks, teacher=False), want)
    order = [5, 16, 0, 3, 11, 2, 9, 1, 14, 7, 4, 13, 6, 15, 8, 10, 12]
    assert_same(sampler.sample_counts(order, 9, "train", batch_tasks=5, teacher=False), [want[i] for i in order])
    for i in (0, 7, 16):                             # a task alone, through the single-draw methods
        b, v, raw, _, mask = sampler.sample_task(i, 9, "train", teacher=False)
        assert (b, tuple(v)) == (want[i][0], tuple(want[i][1]))
        assert np.array_equal(raw, want[i][2]) and np.array_equal(mask, want[i][3])


def test_a_search_that_stops_in_round_one_draws_no_further_round(world):
    sampler, serial = make(world, min_foreground_voxels=1, min_segmentation_volume=1)
    for brain_id, method, kind in (("bare", "sample_bright_voxel", "bright"),
                                   ("annotated", "sample_segmentation_voxel", "segmentation")):
        rng = sampling.TaskRng(3, 0, 11)
        ref.seed_task(3, "train", 11)
        before = sampler.scorer.calls[kind]
        assert getattr(sampler, method)(brain_id, rng) == getattr(serial, method)(brain_id)
        assert sampler.scorer.calls[kind] == before + 1              # one round was scored
        assert rng.py.getstate() == random.getstate()                # and no further voxel drawn
        got, want = rng.np.get_state(), np.random.get_state()
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


def test_the_smallest_label_is_dropped_when_a_patch_holds_no_zero(world):
    for patch in (np.array([[[2, 2, 2, 5, 5, 11]]]),                 # no 0: label 2 is dropped -> 2, not 3
                  np.array([[[0, 2, 2, 2, 5, 5]]]),                  # a 0: nothing positive dropped -> 3
                  np.array([[[4, 4, 4, 4]]]),                        # one value only: no score
                  np.array([[[0, 0, 0]]]), np.array([[[0, 0, 9]]])):
        keys, counts = np.unique(patch[patch > 0], return_counts=True)
        assert sampling.volume_from_label_list(counts, patch.size) == ref.segmentation_score(patch), patch
    assert sampling.volume_from_label_list([3, 2, 1], 6) == 2
    # and through the state machine: the brain at the edge has labels without zeros
    sampler, serial = make({"edge": world["edge"]}, foreground_sampling_rate=1.0)
    want = [serial.sample_counts(4, "train", i) for i in range(12)]
    assert_same(sampler.sample_counts(range(12), 4, "train", teacher=False), want)
    assert sampler.scorer.calls["segmentation"] > 0


class ScriptedScorer(NumpyScorer):
    def __init__(self, *a, script=None, **k):
        super().__init__(*a, **k)
        self.script = list(script)

    def bright(self, brain_id, voxels):
        self.calls["bright"] += 1
        return self.script.pop(0)


def test_the_first_strictly_larger_score_wins(world):
    brains = {"bare": world["bare"]}
    scorer = ScriptedScorer(brains, si.PATCH, script=[[5, 5, 0, 5], [5, 7, 7, 6], [9, 9, 9, 9]])
    p = dict(si.PARAMS, min_foreground_voxels=7)
    sampler = sampling.PatchSampler(sources(brains), si.PATCH, scorer=scorer, **p)
    rng, twin = sampling.TaskRng(1, 0, 0), sampling.TaskRng(1, 0, 0)
    drawn = [sampler.sample_interior_voxel("bare", twin) for _ in range(9)]     # first guess, then 2 x 4
    assert sampler.sample_bright_voxel("bare", rng) == drawn[1 + 4 + 1]         # the first 7, not the second
    assert scorer.calls["bright"] == 2 and len(scorer.script) == 1              # 7 >= 7: no third round
    assert rng.py.getstate() == twin.py.getstate()


def test_exhausted_attempts_return_the_last_draw(world):
    brains = {"annotated": world["annotated"]}
    sampler, serial = make(brains, gate=lambda labels, raw: True, reject_incoherent_patches=True,
                           max_resample_attempts=3, foreground_sampling_rate=0.0)
    rng = sampling.TaskRng(8, 0, 2)
    draws = []
    for _ in range(3):
        b = sampler.sample_brain(rng)
        rng.py.random()
        draws.append((b, sampler.sample_interior_voxel(b, rng)))
    got = sampler.sample_counts([2], 8, "train", teacher=False)
    assert (got[0][0], tuple(got[1][0])) == draws[2]
    assert sampler.scorer.calls["patch"] == 3
    assert_same(got, [serial.sample_counts(8, "train", 2)])


def test_bad_arguments_raise(world, tmp_path):
    src = sources({"bare": world["bare"]})
    with pytest.raises(ValueError):
        sampling.PatchSampler(src, (16, 16), boundary_buffer=12)
    with pytest.raises(ValueError):
        sampling.PatchSampler(src, (16, 0, 16), boundary_buffer=12)
    with pytest.raises(ValueError):
        sampling.PatchSampler({}, si.PATCH, boundary_buffer=12)
    with pytest.raises(ValueError):
        sampling.PatchSampler(src, si.PATCH, boundary_buffer=30)                 # no interior along z
    with pytest.raises(ValueError):
        sampling.BrainSource(None)
    with pytest.raises(ValueError):
        sampling.PatchSampler({"x": None}, si.PATCH, boundary_buffer=12)
    img = world["bare"]["image"][None, None]
    with pytest.raises(ValueError):
        sampling.BrainSource(img[0])                                             # not (1, 1, z, y, x)
    with pytest.raises(ValueError):
        sampling.BrainSource(img, labels=np.zeros((4, 4, 4), np.uint32))
    with pytest.raises(ValueError):
        sampling.BrainSource(img, labels=np.zeros(si.SHAPE, np.float32))
    with pytest.raises(ValueError):
        sampling.BrainSource(img, skeleton=np.zeros((5, 2), np.int64))
    with pytest.raises(ValueError):
        sampling.BrainSource(img, skeleton=np.zeros((5, 3), np.float32))
    sampler, _ = make({"bare": world["bare"]})
    with pytest.raises(ValueError):
        sampler.sample_counts([0], 1, "test")
    with pytest.raises(ValueError):
        sampler.sample_counts([0], 1, "train", batch_tasks=0)
    with pytest.raises(ValueError):
        sampler.skeleton_mask("bare", (20, 20, 20))
    with pytest.raises(ValueError, match="unknown config keys"):
        sampling.precompute_cache(str(tmp_path / "c"), sampler, 2, config={"not_a_key": 1})
    assert not (tmp_path / "c").exists()
