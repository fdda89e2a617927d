"""The sampler's device entries (csrc/sampler_kernels.hip through _native.Context) and machine_learning/sampling.py
end to end on the MI355X, against tests/mask_pyref.py, scipy where it is installed, and the serial restatement
tests/sampling_pyref.py.  Everything is integers, bytes or an existing bit-exact path: every comparison is exact."""
import json
import os

import numpy as np
import pytest

import mask_pyref as P
import sampling_inputs as si
import sampling_pyref as ref
from aind_exaspim_image_compression import _native as nat
from aind_exaspim_image_compression.bm4d import denoise_patches
from aind_exaspim_image_compression.machine_learning import data_handling, metrics, sampling
from aind_exaspim_image_compression.utils import chunk_store

pytestmark = pytest.mark.gpu

try:
    from scipy import ndimage
except ImportError:                                   # the numpy restatement is then the only yardstick
    ndimage = None


# ---- foreground_counts ---------------------------------------------------------------------------------------
def count_batch(dtype, shape, batch, seed):
    """``batch`` patches: noise with bright voxels; patch 1 all above the threshold but one voxel's worth of
    background (a constant patch has nothing above its threshold, so "all above" is every voxel but the median's
    own value), patch 2 constant, patch 3 with a NaN (float32) or saturated values (uint16); the last patch is
    ordinary and dense, so a wrong batch offset shows."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    out = np.empty((batch, n), dtype=np.float64)
    for b in range(batch):
        v = rng.normal(1000.0, 3.0, n)
        v[rng.random(n) < 0.03 + 0.02 * b] += 500.0
        v[b] += 500.0                                 # at least one bright voxel
        out[b] = v
    if batch > 1:
        out[1] = 5000.0
        out[1, : n // 2 + 1] = 100.0                  # the median: everything else is above the threshold
        out[2] = 777.0
        out[3, n // 3] = np.nan if dtype == np.float32 else 65535.0
    return np.clip(np.rint(out), 0, 65535).astype(dtype).reshape((batch,) + shape) if dtype == np.uint16 \
        else out.astype(np.float32).reshape((batch,) + shape)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 20, 36), (1, 1, 70), (9, 1, 65)])
@pytest.mark.parametrize("batch", [1, 5])
def test_foreground_counts(ctx, dtype, shape, batch):
    raw = count_batch(dtype, shape, batch, seed=sum(shape) + batch)
    for dilate in (0, 1, 2, 3):
        with ctx.to_device(raw) as d_raw, ctx.alloc(raw.size) as d_mask:
            got = ctx.foreground_counts(d_raw, raw.dtype, batch, shape, 6.0, dilate)
            ctx.foreground_masks(d_raw, raw.dtype, batch, shape, 6.0, dilate, d_mask)
            masks = d_mask.download(raw.shape, np.uint8)
        what = f"{np.dtype(dtype).name} {shape} batch {batch} dilate {dilate}"
        assert got.dtype == np.uint32
        want = [int(P.fg_mask(p, 6.0, dilate).sum()) for p in raw]
        print(what, got.tolist())
        assert got.tolist() == [int(m.sum()) for m in masks], what
        assert got.tolist() == want, what
        if ndimage is not None:
            for b, p in enumerate(raw):
                m = np.asarray(p, np.float32) > P.fg_threshold(p, 6.0)
                if dilate:
                    m = ndimage.binary_dilation(m, iterations=dilate)
                assert int(got[b]) == int(m.sum()), what
        if batch > 1:
            n = int(np.prod(shape))
            assert got[2] == 0, what                                  # constant
            if dtype == np.float32:
                assert got[3] == 0 and got[4] > 0 and got[0] > 0, what   # the NaN patch, and its neighbours
            if dilate == 0:
                assert got[1] == n - (n // 2 + 1), what               # everything but the median's value


def test_foreground_counts_refuses_bad_arguments(ctx):
    raw = np.zeros((1, 4, 4, 4), np.float32)
    with ctx.to_device(raw) as d:
        with pytest.raises(ValueError):
            ctx.foreground_counts(d, np.float32, 1, (4, 4, 4), 6.0, -1)
        with pytest.raises(ValueError):
            ctx.foreground_counts(d, np.float32, 0, (4, 4, 4))
        with pytest.raises(ValueError):
            ctx.foreground_counts(None, np.float32, 1, (4, 4, 4))


# ---- annotation_masks ----------------------------------------------------------------------------------------
def annotation_run(ctx, labels, points, starts, shape, seg_dilate, skel_dilate):
    """The entry on host arrays; the mask buffer comes poisoned, so every byte must have been written."""
    batch = len(starts)
    d_labels = ctx.to_device(labels) if labels is not None else None
    d_points = None
    if points is not None:
        d_points = ctx.to_device(points.astype(np.int32) if len(points) else np.zeros((1, 3), np.int32))
    d_mask = ctx.to_device(np.full(batch * int(np.prod(shape)), 0xAB, np.uint8))
    try:
        ctx.annotation_masks(d_labels, labels.dtype if labels is not None else np.uint8, seg_dilate, d_points,
                             0 if points is None else len(points), starts, skel_dilate, shape, d_mask)
        return d_mask.download((batch,) + tuple(shape), np.uint8)
    finally:
        for d in (d_labels, d_points, d_mask):
            if d is not None:
                d.free()


def annotation_want(labels, points, starts, shape, seg_dilate, skel_dilate):
    out = []
    for b, start in enumerate(starts):
        m = np.zeros(shape, bool)
        if labels is not None:
            m |= P.dilate(labels[b] > 0, seg_dilate)
        if points is not None:
            m |= ref.skeleton_mask(points.reshape(-1, 3), start, shape, skel_dilate)
        out.append(m)
    return np.stack(out).astype(np.uint8)


def face_points(start, shape):
    """Every corner and a point on every face of the box, the same just outside, and duplicates."""
    s, e = np.array(start), np.array(start) + np.array(shape) - 1
    pts = [[z, y, x] for z in (s[0], e[0]) for y in (s[1], e[1]) for x in (s[2], e[2])]
    mid = (s + e) // 2
    for ax in range(3):
        for v, step in ((s[ax], -1), (e[ax], 1)):
            p = mid.copy()
            p[ax] = v
            pts.append(p.tolist())
            p[ax] = v + step                          # just outside
            pts.append(p.tolist())
    pts += [[s[0] - 1, s[1] - 1, s[2] - 1], [e[0] + 1, e[1] + 1, e[2] + 1]]
    return np.array(pts + pts[:5], dtype=np.int64)


@pytest.mark.parametrize("label_dtype", [np.uint8, np.uint32, np.uint64, np.int32, None])
@pytest.mark.parametrize("dilations", [(0, 0), (2, 2), (0, 2)])
def test_annotation_masks(ctx, label_dtype, dilations):
    rng = np.random.default_rng(11)
    shape = (9, 12, 21)
    starts = np.array([[10, 10, 10], [14, 16, 20], [-3, 5, 100], [10, 10, 10], [500, 500, 500], [0, 0, 0]])
    labels = None
    if label_dtype is not None:
        labels = (rng.random((len(starts),) + shape) < 0.02) * rng.integers(1, 200, (len(starts),) + shape)
        labels = labels.astype(label_dtype)
        if label_dtype == np.int32:
            labels[rng.random(labels.shape) < 0.05] = -7             # negative ids are background
        if label_dtype == np.uint64:
            labels[labels > 0] += np.uint64(1) << np.uint64(40)
    cloud = np.concatenate([face_points(starts[0], shape), face_points(starts[2], shape),
                            rng.integers(0, 40, (300, 3)),            # boxes 2 and 4 lie partly / wholly outside it
                            np.array([[15, 17, 22]])])                # inside the overlapping boxes 0, 1 and 3
    for name, points in (("none", None), ("empty", np.zeros((0, 3), np.int64)), ("cloud", cloud)):
        if labels is None and points is None:
            continue
        got = annotation_run(ctx, labels, points, starts, shape, *dilations)
        want = annotation_want(labels, points, starts, shape, *dilations)
        assert np.array_equal(got, want), (name, label_dtype, dilations)
        if points is cloud and dilations[1] == 0 and labels is None:
            assert got[0, 5, 7, 12] == 1 and got[1, 1, 1, 2] == 1 and got[3, 5, 7, 12] == 1
            assert got[4].sum() == 0 and got[0].sum() > 20


def test_annotation_masks_of_more_boxes_than_one_launch_holds(ctx):
    rng = np.random.default_rng(12)
    batch, shape = nat.RASTER_BOXES + 44, (8, 8, 8)
    starts = rng.integers(-4, 60, (batch, 3))
    starts[nat.RASTER_BOXES:] += 100                  # the second launch has a bounding box of its own
    points = np.concatenate([rng.integers(-4, 68, (4000, 3)), rng.integers(96, 168, (3000, 3))])
    labels = ((rng.random((batch,) + shape) < 0.01) * 5).astype(np.uint32)
    for lab in (None, labels):
        for dil in (0, 2):
            got = annotation_run(ctx, lab, points, starts, shape, 0, dil)
            assert np.array_equal(got, annotation_want(lab, points, starts, shape, 0, dil)), (lab is None, dil)
    assert got[-1].sum() > 0 and got[nat.RASTER_BOXES].sum() > 0


def test_annotation_masks_refuses_bad_arguments(ctx):
    starts = np.zeros((1, 3), np.int32)
    with ctx.alloc(64) as d_mask, ctx.to_device(np.zeros((1, 4, 4, 4), np.uint8)) as d_lab:
        with pytest.raises(ValueError):
            ctx.annotation_masks(None, np.uint8, 0, None, 0, starts, 0, (4, 4, 4), d_mask)      # no annotation
        with pytest.raises(ValueError):
            ctx.annotation_masks(d_lab, np.uint8, -1, None, 0, starts, 0, (4, 4, 4), d_mask)
        with pytest.raises(ValueError):
            ctx.annotation_masks(d_lab, np.uint8, 0, None, 0, starts, 0, (4, 4, 4), None)


# ---- end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    root = tmp_path_factory.mktemp("sampling")
    brains = si.brains()
    srcs = {}
    for name, b in brains.items():
        paths = {}
        for key in ("image", "val_image"):
            paths[key] = str(root / f"{name}_{key}")
            chunk_store.write_zarr(b[key], paths[key], (1, 1, 32, 32, 32))
        srcs[name] = sampling.BrainSource(chunk_store.open_zarr(paths["image"]), labels=b["labels"],
                                          skeleton=b["skeleton"], offset=b["offset"],
                                          val_image=chunk_store.open_zarr(paths["val_image"]))
    return brains, srcs


def gate(labels, raw):
    return metrics.patch_has_incoherent_segment(labels, raw)


E2E = dict(si.PARAMS, reject_incoherent_patches=True, max_resample_attempts=4, sigma_bm4d=24)


@pytest.fixture(scope="module")
def drawn(stores):
    """(sampler, {split: what sample_counts drew for 12 tasks}), computed once."""
    brains, srcs = stores
    assert E2E["boundary_buffer"] == 12 and E2E["prefetch_foreground_sampling"] == 4 and si.PATCH == (16, 16, 16)
    sampler = sampling.PatchSampler(srcs, si.PATCH, **E2E)
    return sampler, {split: sampler.sample_counts(range(12), 42, split, batch_tasks=7) for split in ("train", "val")}


@pytest.mark.parametrize("split", ["train", "val"])
def test_sample_counts_equals_the_serial_reference(stores, drawn, split):
    brains, _ = stores
    serial = ref.RefSampler(brains, si.PATCH, gate=gate,
                            **{k: v for k, v in E2E.items() if k != "sigma_bm4d"})
    sampler, got = drawn
    brain_ids, voxels, raw, teacher, masks = got[split]
    for i in range(12):
        b, v, r, m = serial.sample_counts(42, split, i)
        assert (brain_ids[i], tuple(voxels[i])) == (b, tuple(v)), i
        assert np.array_equal(raw[i], r) and np.array_equal(masks[i], m), i
    assert set(brain_ids) == set(brains)
    assert teacher.dtype == np.float32
    assert np.array_equal(teacher, denoise_patches(raw, sigma=24.0, max_count=float(sampler.transform.max_count)))
    one = sampler.sample_counts(range(12), 42, split, batch_tasks=1, teacher=False)
    assert one[0] == brain_ids and np.array_equal(one[1], voxels)
    assert np.array_equal(one[2], raw) and np.array_equal(one[4], masks)
    b, v, r, _, m = sampler.sample_task(5, 42, split, teacher=False)      # alone, through the single draws
    assert (b, tuple(v)) == (brain_ids[5], tuple(voxels[5])) and np.array_equal(r, raw[5]) and np.array_equal(m, masks[5])


@pytest.mark.parametrize("split", ["train", "val"])
def test_precompute_cache_is_read_back_by_the_cached_dataset(drawn, tmp_path, split):
    sampler, got = drawn
    _, _, raw, teacher, masks = got[split]
    cache = str(tmp_path / split)
    sampling.precompute_cache(cache, sampler, 12, split=split, seed=42, batch_tasks=5,
                              config={"num_workers": 1})
    ds = data_handling.CachedPatchDataset(cache, transform=sampler.transform)
    assert len(ds) == 12
    for i in range(12):
        r, t, f = ds._get_arrays(i)
        assert np.array_equal(r, raw[i]) and np.array_equal(t, teacher[i]) and np.array_equal(f, masks[i]), i
    with open(os.path.join(cache, "config.json")) as f:
        cfg = json.load(f)
    assert set(cfg) == set(data_handling.CONFIG_KEYS)
    for key, value in sampler.config().items():
        assert cfg[key] == value, key
    assert cfg["split"] == split and cfg["seed"] == 42 and cfg["seed_stream"] == data_handling.SEED_STREAMS[split]
    assert cfg["n_patches"] == 12 and cfg["patch_shape"] == list(si.PATCH) and cfg["num_workers"] == 1
    assert cfg["reject_incoherent_patches"] is True and cfg["max_resample_attempts"] == 4
    stamps = {n: os.stat(os.path.join(cache, n)).st_mtime_ns for n in os.listdir(cache)}
    assert stamps["transform.json"] == max(stamps.values())                  # written last
    assert data_handling.load_cached_transform(cache, cache).cfg == sampler.transform.cfg
