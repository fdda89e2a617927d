"""Label stores on the MI355X: ``write_zarr`` / ``read_zarr`` / ``read_chunk`` with ``LabelCodec``, ``LabelArray``
region reads against numpy slicing and the zero-fill rule, whole-chunk region writes, and the samplers reading their
labels from a store.  Integer data: every comparison is exact."""
import os

import numpy as np
import pytest

import label_pyref as ref
import sampling_inputs as si
from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import sampling
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.label_codec import LabelCodec
from aind_exaspim_image_compression.utils.store_labels import LabelArray
from aind_exaspim_image_compression.utils.store_read import DevicePatches

pytestmark = pytest.mark.gpu

DTYPES = (np.uint32, np.uint64)
SHAPE, CHUNKS = (40, 24, 19), (1, 1, 16, 16, 16)


def volume(dtype):
    """The class-boundary volume with tubes laid over its empty part: every block class, and structure everywhere."""
    vol = ref.class_volume(SHAPE, dtype)
    tubes = ref.tube_volume(SHAPE, dtype)
    return np.where(vol == 0, tubes, vol)


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """dtype name -> (volume, path of its store), written once."""
    root = tmp_path_factory.mktemp("labels")
    out = {}
    for dtype in DTYPES:
        vol = volume(dtype)
        path = str(root / np.dtype(dtype).name)
        ratio = chunk_store.write_zarr(vol, path, CHUNKS, codec=LabelCodec(vol.dtype.itemsize))
        assert ratio > 1.0
        vol.setflags(write=False)
        out[np.dtype(dtype).name] = (vol, path)
    return out


def zero_filled(vol, starts, box):
    """``read_label_patches``' rule, by numpy."""
    out = np.zeros((len(starts),) + tuple(box), dtype=vol.dtype)
    for n, start in enumerate(starts):
        lo = np.clip(start, 0, vol.shape)
        hi = np.clip(np.asarray(start) + np.array(box), 0, vol.shape)
        if np.all(hi > lo):
            src = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
            dst = tuple(slice(int(a - s), int(b - s)) for a, b, s in zip(lo, hi, start))
            out[n][dst] = vol[src]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_read_round_trip_and_chunks(stores, dtype):
    vol, path = stores[np.dtype(dtype).name]
    back = chunk_store.read_zarr(path)
    assert back.shape == (1, 1) + SHAPE and back.dtype == vol.dtype and np.array_equal(back[0, 0], vol)
    for idx in ((0, 0, 0), (1, 0, 0), (2, 1, 1), (0, 1, 1)):       # interior and corner chunks
        sl = tuple(slice(16 * i, 16 * i + 16) for i in idx)
        got = chunk_store.read_chunk(path, *idx)
        assert got.dtype == vol.dtype and np.array_equal(got, vol[sl]), idx
        with open(os.path.join(path, chunk_store.chunk_key(*idx)), "rb") as f:
            assert f.read() == ref.encode(vol[sl]), idx
    with pytest.raises(IndexError):
        chunk_store.read_chunk(path, 3, 0, 0)
    enc, meta = chunk_store.read_encoded(path)
    assert meta["data_type"] == vol.dtype.name and enc.typesize == vol.dtype.itemsize
    chunk_store.write_encoded(enc, path + "_copy", codec=LabelCodec(vol.dtype.itemsize))
    assert np.array_equal(chunk_store.read_zarr(path + "_copy")[0, 0], vol)


@pytest.mark.parametrize("dtype", DTYPES)
def test_getitem_against_numpy(stores, dtype):
    vol, path = stores[np.dtype(dtype).name]
    arr = chunk_store.open_zarr(path)
    assert isinstance(arr, LabelArray) and arr.dtype == vol.dtype
    full = vol[None, None]
    keys = [(0, 0, 5, 6, 7), (0, 0, 39, 23, 18), (0, 0, -1, -1, -1),                       # single voxels
            (0, 0, slice(7, 17), slice(7, 17), slice(7, 17)),                               # start 7, length 10
            (0, 0, slice(15, 33), slice(1, 24), slice(3, 19)), (0, 0, slice(31, 40), slice(15, 17), slice(15, 19)),
            (0, 0, 17), (0, 0, slice(None), 9), (0, 0, slice(None), slice(None), 16),       # full planes
            (slice(None), slice(None), slice(8, 9)), (0, 0), (0, 0, slice(5, 5))]
    for key in keys:
        got, want = arr[key], full[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        assert np.array_equal(got, want), key
    for bad in ((0, 0, slice(0, 8, 2)), (0, 0, 40), (1,), (0, 0, Ellipsis)):
        with pytest.raises(IndexError):
            arr[bad]


@pytest.mark.parametrize("dtype", DTYPES)
def test_read_patches_against_the_zero_fill_rule(stores, dtype):
    vol, path = stores[np.dtype(dtype).name]
    arr = chunk_store.open_zarr(path)
    rng = np.random.default_rng(3)
    box = (12, 9, 17)
    starts = np.stack([rng.integers(0, s - b + 1, 50) for s, b in zip(SHAPE, box)], axis=1)
    over = [(-5, 3, 1), (33, 3, 1), (10, -4, 1), (10, 19, 1), (10, 3, -9), (10, 3, 11),      # every face
            (-5, -4, -9), (35, 20, 12), (-12, 0, 0), (40, 0, 0), (100, 100, 100), (-50, 3, 1)]  # corners, outside
    starts = np.concatenate([starts, np.array(over)])
    want = zero_filled(vol, starts, box)
    assert not want[-1].any() and not want[-2].any() and want[:50].any()
    got = arr.read_patches(starts, box, is_center=False)
    assert got.dtype == vol.dtype and got.shape == want.shape
    assert np.array_equal(got, want)
    assert arr.last_read["groups"] == 1 and arr.last_read["gather_calls"] == 1
    assert arr.last_read["chunks"] == 3 * 2 * 2 and arr.last_read["chunk_bytes"] > 0
    dev = arr.read_patches(starts, box, is_center=False, out="device")
    try:
        assert isinstance(dev, DevicePatches) and dev.shape == want.shape and dev.dtype == vol.dtype
        assert np.array_equal(dev.download(), want)
    finally:
        dev.free()
    # centred boxes: box n starts at voxel - d // 2
    centred = arr.read_patches(starts + np.array([d // 2 for d in box]), box)
    assert np.array_equal(centred, want)
    # several groups under a tiny cap on the coded bytes give the same patches
    small = chunk_store.open_zarr(path, max_pool_bytes=2000)
    assert np.array_equal(small.read_patches(starts, box, is_center=False), want)
    assert small.last_read["groups"] > 4 and small.last_read["gather_calls"] == small.last_read["groups"]
    empty = arr.read_patches(np.zeros((0, 3), np.int64), box, out="device")
    assert empty.shape == (0,) + box and empty.data_ptr() == 0
    # a 64^3 patch over a store of smaller chunks: more chunks per box than any case above
    big = arr.read_patches([(20, 12, 9)], (64, 64, 64))
    assert np.array_equal(big, zero_filled(vol, [(-12, -20, -23)], (64, 64, 64)))


def test_a_missing_chunk_raises(stores, tmp_path):
    vol, path = stores["uint64"]
    other = str(tmp_path / "holes")
    enc, _ = chunk_store.read_encoded(path)
    chunk_store.write_encoded(enc, other, codec=LabelCodec(8))
    os.remove(os.path.join(other, chunk_store.chunk_key(1, 1, 0)))
    arr = chunk_store.open_zarr(other)
    assert np.array_equal(arr[0, 0, 0:16, 0:16, 0:16], vol[0:16, 0:16, 0:16])
    with pytest.raises(FileNotFoundError):
        arr[0, 0, 16:20, 16:20, 0:4]
    assert arr.last_read is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_slab_by_slab_writes_equal_write_zarr(stores, tmp_path, dtype):
    vol, path = stores[np.dtype(dtype).name]
    made = str(tmp_path / "slabs")
    arr = chunk_store.create_zarr(made, SHAPE, CHUNKS, codec=LabelCodec(vol.dtype.itemsize))
    assert isinstance(arr, LabelArray) and arr.mode == "r+"
    for z0 in (0, 16, 32):                                          # the last slab ends at the array's edge
        arr[0, 0, z0:min(z0 + 16, 40), :, 0:16] = vol[z0:z0 + 16, :, 0:16]
        assert arr.last_write["encode_calls"] == 1 and arr.last_write["chunks"] == 2
    arr[0, 0, :, :, 16:19] = vol[:, :, 16:19]                       # the truncated column of chunks, in one write
    assert arr.last_write["chunks"] == 6
    for dirpath, _, files in os.walk(path):
        for name in files:
            a = os.path.join(dirpath, name)
            b = os.path.join(made, os.path.relpath(a, path))
            if name == "zarr.json":
                continue
            with open(a, "rb") as fa, open(b, "rb") as fb:
                assert fa.read() == fb.read(), os.path.relpath(a, path)
    assert sum(len(f) for _, _, f in os.walk(path)) == sum(len(f) for _, _, f in os.walk(made))
    assert np.array_equal(chunk_store.open_zarr(made)[0, 0], vol)
    arr[0, 0, 16:32, 0:16, 0:16] = 5                                # a scalar fills whole chunks
    assert np.all(arr[0, 0, 16:32, 0:16, 0:16] == 5) and np.array_equal(arr[0, 0, 0:16], vol[0:16])
    with pytest.raises(ValueError):
        arr[0, 0, 0:16, 0:16, 0:15] = vol[0:16, 0:16, 0:15]


# ---- the samplers ---------------------------------------------------------------------------------------------
E2E = dict(si.PARAMS, reject_incoherent_patches=True, max_resample_attempts=4, sigma_bm4d=24)


@pytest.fixture(scope="module")
def samplers(tmp_path_factory):
    """(brains, a sampler over numpy labels, the same over a label store)."""
    root = tmp_path_factory.mktemp("label_sampling")
    brains = si.brains()
    by_kind = {"numpy": {}, "store": {}}
    for name, b in brains.items():
        paths = {}
        for key in ("image", "val_image"):
            paths[key] = str(root / f"{name}_{key}")
            chunk_store.write_zarr(b[key], paths[key], (1, 1, 32, 32, 32))
        store = None
        if b["labels"] is not None:
            chunk_store.write_zarr(b["labels"], str(root / f"{name}_labels"), (1, 1, 32, 32, 32),
                                   codec=LabelCodec(b["labels"].dtype.itemsize))
            store = chunk_store.open_zarr(str(root / f"{name}_labels"))
            assert isinstance(store, LabelArray)
        for kind, labels in (("numpy", b["labels"]), ("store", store)):
            by_kind[kind][name] = sampling.BrainSource(
                chunk_store.open_zarr(paths["image"]), labels=labels, skeleton=b["skeleton"], offset=b["offset"],
                val_image=chunk_store.open_zarr(paths["val_image"]))
    return (brains, sampling.PatchSampler(by_kind["numpy"], si.PATCH, **E2E),
            sampling.PatchSampler(by_kind["store"], si.PATCH, **E2E))


def test_brain_source_checks_a_label_store_against_the_image(samplers, tmp_path):
    _, plain, stored = samplers
    image = plain.brains["annotated"].image
    labels = stored.brains["annotated"].labels
    assert labels.shape == (1, 1) + si.SHAPE
    other = chunk_store.create_zarr(str(tmp_path / "small"), (8, 8, 8), codec=LabelCodec(4))
    with pytest.raises(ValueError):
        sampling.BrainSource(image, labels=other)


@pytest.mark.parametrize("split", ["train", "val"])
def test_samplers_draw_the_same_from_a_label_store(samplers, split):
    brains, plain, stored = samplers
    want = plain.sample_counts(range(12), 42, split, batch_tasks=7, teacher=False)
    got = stored.sample_counts(range(12), 42, split, batch_tasks=7, teacher=False)
    assert got[0] == want[0] and "annotated" in got[0]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
    for index in (0, 5, 11):                                        # alone, through the single draws
        a = plain.sample_task(index, 42, split, teacher=False)
        b = stored.sample_task(index, 42, split, teacher=False)
        assert (a[0], tuple(a[1])) == (b[0], tuple(b[1])) == (want[0][index], tuple(want[1][index]))
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]) and np.array_equal(b[4], want[4][index])


def test_single_draws_from_a_label_store(samplers):
    brains, plain, stored = samplers
    labels = brains["annotated"]["labels"]
    for seed in range(4):
        a = plain.sample_segmentation_voxel("annotated", rng=sampling.TaskRng(seed, 0, 1))
        b = stored.sample_segmentation_voxel("annotated", rng=sampling.TaskRng(seed, 0, 1))
        assert a == b
    for centre in ((24, 30, 40), (30, 44, 24), (16, 48, 54), (2, 3, 4), (47, 63, 79)):
        want = plain.annotation_mask("annotated", centre)
        assert np.array_equal(stored.annotation_mask("annotated", centre), want)
        patch = stored.scorer.labels("annotated", [centre])
        assert patch.dtype == labels.dtype
        assert np.array_equal(patch, sampling.read_label_patches(labels, [centre], si.PATCH))
    for seed in range(3):
        a = plain.sample_clean(rng=sampling.TaskRng(seed, 1, 2))
        b = stored.sample_clean(rng=sampling.TaskRng(seed, 1, 2))
        assert (a[0], a[1]) == (b[0], b[1]) and np.array_equal(a[2], b[2])
        assert (a[3] is None and b[3] is None) or np.array_equal(a[3], b[3])


def test_segmentation_scores_upload_no_labels(samplers, monkeypatch):
    """``DeviceScorer.segmentation`` of a label store hands the gathered patches to ``label_set`` where they lie: the
    only uploads are the coded bytes."""
    brains, plain, stored = samplers
    rng = np.random.default_rng(9)
    voxels = [tuple(int(rng.integers(8, s - 8)) for s in si.SHAPE) for _ in range(20)] + [(24, 30, 40), (30, 44, 24)]
    want = plain.scorer.segmentation("annotated", voxels)
    assert any(w is not None and w > 0 for w in want)
    uploads = []
    real = _native.Context.to_device

    def counted(self, arr):
        uploads.append((np.asarray(arr).dtype, np.asarray(arr).size))
        return real(self, arr)

    monkeypatch.setattr(_native.Context, "to_device", counted)
    got = stored.scorer.segmentation("annotated", voxels)
    assert got == want
    assert uploads and all(dt == np.uint8 for dt, _ in uploads), uploads
    uploads.clear()
    plain.scorer.segmentation("annotated", voxels)                  # the host path does upload its label patches
    assert any(dt == np.uint32 and n == len(voxels) * int(np.prod(si.PATCH)) for dt, n in uploads)
    uploads.clear()
    masks = stored.scorer.annotation_masks("annotated", voxels, stored.scorer.labels("annotated", voxels))
    assert uploads and not any(dt in (np.uint32, np.uint64) for dt, _ in uploads), uploads   # no label patch
    monkeypatch.undo()
    assert np.array_equal(masks, plain.scorer.annotation_masks(
        "annotated", voxels, plain.scorer.labels("annotated", voxels)))
