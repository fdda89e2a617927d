"""Label stores, the host side (no GPU): the read planner against a brute-force enumeration, ``zarr.json`` of both
typesizes, what opens as what, the refusals that must come before a byte is written, and corrupt chunk files rejected
before any device call."""
import json
import os
import struct

import numpy as np
import pytest

import label_pyref as ref
from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store, label_codec
from aind_exaspim_image_compression.utils.label_codec import LabelCodec
from aind_exaspim_image_compression.utils.store_labels import LabelArray, plan_label_read
from aind_exaspim_image_compression.utils.store_read import StoredArray


def touched(shape, chunk, start, box):
    """Chunk indices a box touches, by enumerating its voxels' chunks axis by axis."""
    per_axis = []
    for s, c, a, b in zip(shape, chunk, start, box):
        per_axis.append(sorted({v // c for v in range(max(int(a), 0), min(int(a) + b, s))}))
    return [(z, y, x) for z in per_axis[0] for y in per_axis[1] for x in per_axis[2]]


def check_plan(groups, shape, chunk, box, starts):
    assert [g.first for g in groups] == [0] + [g.stop for g in groups[:-1]] and groups[-1].stop == len(starts)
    for g in groups:
        want = sorted({t for n in range(g.first, g.stop) for t in touched(shape, chunk, starts[n], box)})
        assert [tuple(int(v) for v in c) for c in g.chunks] == want
        assert g.box_srcs.shape[0] == g.stop - g.first and g.box_srcs.dtype == np.int32
        for n in range(g.first, g.stop):
            row = g.box_srcs[n - g.first]
            mine = touched(shape, chunk, starts[n], box)            # raster order over the box's chunk range
            assert [tuple(int(v) for v in g.chunks[m]) for m in row[:len(mine)]] == mine
            assert np.all(row[len(mine):] == -1)


def test_planner_random_boxes_inside_partly_and_wholly_outside():
    rng = np.random.default_rng(5)
    for _ in range(60):
        chunk = tuple(int(c) for c in rng.integers(1, 9, 3))
        shape = tuple(int(s) for s in rng.integers(1, 30, 3))
        box = tuple(int(b) for b in rng.integers(1, 40, 3))
        n = int(rng.integers(1, 6))
        starts = np.stack([rng.integers(-box[a] - 3, shape[a] + 4, n) for a in range(3)], axis=1)
        groups = plan_label_read(shape, chunk, starts, box, lambda idx: 100)
        assert len(groups) == 1
        check_plan(groups, shape, chunk, box, starts)


def test_planner_groups_under_the_cap_on_coded_bytes():
    shape, chunk, box = (32, 32, 32), (8, 8, 8), (8, 8, 8)
    starts = np.array([(0, 0, 0), (0, 0, 0), (8, 0, 0), (16, 0, 0), (40, 40, 40), (4, 4, 4)])
    size = {}

    def coded(idx):
        size[idx] = 1000 if idx == (1, 0, 0) else 90         # 90 pads to 96
        return size[idx]

    groups = plan_label_read(shape, chunk, starts, box, coded, max_pool_bytes=1 << 30)
    assert len(groups) == 1 and groups[0].coded_bytes == 96 * 8 + 1008      # nine chunks, one of them large
    check_plan(groups, shape, chunk, box, starts)
    # a box costs 12 + 4 per chunk, a chunk 40 + its padded stream; a chunk held by the group is not counted again
    one = 12 + 4 + 40 + 96
    groups = plan_label_read(shape, chunk, starts, box, coded, max_pool_bytes=one + 16 + 100)
    assert [(g.first, g.stop) for g in groups] == [(0, 2), (2, 3), (3, 5), (5, 6)]
    check_plan(groups, shape, chunk, box, starts)
    assert [g.coded_bytes for g in groups] == [96, 1008, 96, 96 * 7 + 1008]
    # a cap below one box's needs: one group per box
    groups = plan_label_read(shape, chunk, starts, box, coded, max_pool_bytes=1)
    assert [(g.first, g.stop) for g in groups] == [(n, n + 1) for n in range(len(starts))]
    # the box wholly outside touches nothing
    assert groups[4].chunks.shape == (0, 3) and np.all(groups[4].box_srcs == -1)


def test_planner_empty_batch_and_bad_sizes():
    assert plan_label_read((8, 8, 8), (4, 4, 4), np.zeros((0, 3), np.int64), (2, 2, 2), lambda idx: 1) == []
    with pytest.raises(ValueError):
        plan_label_read((8, 8, 8), (4, 4, 0), [(0, 0, 0)], (2, 2, 2), lambda idx: 1)
    with pytest.raises(ValueError):
        plan_label_read((8, 8), (4, 4), [(0, 0, 0)], (2, 2, 2), lambda idx: 1)


# ---- metadata ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typesize,name", [(4, "uint32"), (8, "uint64")])
def test_metadata_round_trip(typesize, name):
    meta = chunk_store.metadata((40, 24, 19), (16, 16, 16), codec=LabelCodec(typesize))
    assert meta["data_type"] == name and meta["codecs"][0]["name"] == "exac-labels"
    meta = json.loads(json.dumps(meta))
    assert chunk_store.check_metadata(meta) == ((40, 24, 19), (16, 16, 16), typesize, False)
    codec = chunk_store._codec_of(meta)
    assert isinstance(codec, LabelCodec) and codec.typesize == typesize
    assert codec.config_entry() == LabelCodec(typesize).config_entry()


def test_data_type_mapping_of_the_other_codecs_is_unchanged():
    assert chunk_store.metadata((8, 8, 8), (8, 8, 8), typesize=2)["data_type"] == "uint16"
    assert chunk_store.metadata((8, 8, 8), (8, 8, 8), typesize=4)["data_type"] == "int32"
    meta = chunk_store.metadata((8, 8, 8), (8, 8, 8), typesize=4)
    for wrong in ("uint64", "uint32"):
        with pytest.raises(ValueError):
            chunk_store.check_metadata(dict(meta, data_type=wrong))
    labels = chunk_store.metadata((8, 8, 8), (8, 8, 8), codec=LabelCodec(4))
    for wrong in ("int32", "uint16", "uint64"):
        with pytest.raises(ValueError):
            chunk_store.check_metadata(dict(labels, data_type=wrong))
    for cfg in ({"version": 2, "typesize": 8, "edge_chunks": "truncated"},
                {"version": 1, "typesize": 2, "edge_chunks": "truncated"}, {"version": 1, "typesize": 8}):
        bad = dict(labels, codecs=[{"name": "exac-labels", "configuration": cfg}])
        with pytest.raises(ValueError):
            chunk_store.check_metadata(bad)
    with pytest.raises(ValueError):
        LabelCodec(2)


def pyref_store(path, vol, chunk):
    """A label store written without the GPU: the pyref's streams under ``chunk_store``'s own metadata."""
    ts = vol.dtype.itemsize
    chunk = tuple(min(c, s) for c, s in zip(chunk, vol.shape))
    os.makedirs(path)
    grid = [-(-s // c) for s, c in zip(vol.shape, chunk)]
    for iz in range(grid[0]):
        for iy in range(grid[1]):
            for ix in range(grid[2]):
                sub = vol[iz * chunk[0]:(iz + 1) * chunk[0], iy * chunk[1]:(iy + 1) * chunk[1],
                          ix * chunk[2]:(ix + 1) * chunk[2]]
                final = os.path.join(path, chunk_store.chunk_key(iz, iy, ix))
                os.makedirs(os.path.dirname(final), exist_ok=True)
                with open(final, "wb") as f:
                    f.write(ref.encode(sub))
    with open(os.path.join(path, "zarr.json"), "w") as f:
        json.dump(chunk_store.metadata(vol.shape, chunk, codec=LabelCodec(ts)), f)
    return path


def test_open_zarr_returns_the_array_of_the_stores_codec(tmp_path):
    vol = ref.class_volume((16, 16, 11), np.uint32, counts=(1, 3, 17, 512))
    arr = chunk_store.open_zarr(pyref_store(str(tmp_path / "labels"), vol, (8, 8, 8)))
    assert isinstance(arr, LabelArray)
    assert arr.shape == (1, 1, 16, 16, 11) and arr.chunks == (1, 1, 8, 8, 8) and arr.dtype == np.uint32
    assert arr.ndim == 5 and len(arr) == 1 and arr.mode == "r"
    os.makedirs(tmp_path / "image")
    with open(tmp_path / "image" / "zarr.json", "w") as f:
        json.dump(chunk_store.metadata((16, 16, 11), (8, 8, 8)), f)
    assert isinstance(chunk_store.open_zarr(str(tmp_path / "image")), StoredArray)
    with pytest.raises(ValueError):
        chunk_store.open_zarr(str(tmp_path / "labels"), codec=LabelCodec(8))
    with pytest.raises(ValueError):
        LabelArray(str(tmp_path / "image"))


def test_create_zarr_and_refusals_before_a_byte_is_written(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was attempted")

    monkeypatch.setattr(_native, "context", no_device)
    path = str(tmp_path / "made")
    arr = chunk_store.create_zarr(path, (40, 24, 19), chunks=(1, 1, 16, 16, 16), codec=LabelCodec(8))
    assert isinstance(arr, LabelArray) and arr.mode == "r+" and arr.dtype == np.uint64
    assert arr.shape == (1, 1, 40, 24, 19) and arr.chunks == (1, 1, 16, 16, 16)
    before = sorted(os.listdir(path))
    block = np.ones((16, 16, 16), np.uint64)
    for key, value in (((0, 0, slice(0, 16), slice(0, 16), slice(1, 17)), block),        # off the grid
                       ((0, 0, slice(0, 15), slice(0, 16), slice(0, 16)), block[:15]),     # ends inside a chunk
                       ((0, 0, slice(8, 24), slice(0, 16), slice(0, 16)), block),          # starts inside a chunk
                       ((0, 0, slice(0, 16), slice(0, 16), slice(0, 16)), block[:8]),      # a value of another shape
                       ((0, 0, slice(0, 16), slice(0, 16), slice(0, 16)), block.astype(np.float32)),
                       ((0, 0, slice(0, 16), slice(0, 16), slice(0, 16)), -block.astype(np.int64))):
        with pytest.raises(ValueError):
            arr[key] = value
    assert sorted(os.listdir(path)) == before
    with pytest.raises(ValueError):
        chunk_store.open_zarr(path)[0, 0, 0:16, 0:16, 0:16] = block          # read-only
    with pytest.raises(FileExistsError):
        chunk_store.create_zarr(path, (40, 24, 19), chunks=(1, 1, 16, 16, 16), codec=LabelCodec(8))
    # the other codecs' refusal stays
    with pytest.raises(NotImplementedError):
        chunk_store.create_zarr(str(tmp_path / "idx"), (8, 8, 8), codec=chunk_store.ExacCodec(4))
    # and uint16 voxels are no labels
    with pytest.raises(ValueError):
        chunk_store.write_zarr(np.zeros((8, 8, 8), np.uint16), str(tmp_path / "u16"), codec=LabelCodec(8))
    with pytest.raises(ValueError):
        chunk_store.write_zarr(np.zeros((8, 8, 8), np.uint32), str(tmp_path / "u32"), codec=LabelCodec(8))
    assert not os.path.exists(tmp_path / "u16") and not os.path.exists(tmp_path / "u32")


# ---- corrupt chunk files ------------------------------------------------------------------------------------------
def _patched(blob, at, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, *values)
    return bytes(b)


def corruptions(blob):
    nblocks = struct.unpack_from("<I", blob, 20)[0]
    at, k, bits = ref.table(blob)
    mixed = int(np.flatnonzero(bits == 2)[0])
    return {
        "magic": _patched(blob, 0, "<4s", b"EXAC"),
        "version": _patched(blob, 4, "<H", 3),
        "typesize": _patched(blob, 6, "<H", 12 - struct.unpack_from("<H", blob, 6)[0]),
        "extent": _patched(blob, 16, "<I", 7),
        "offset past the end": _patched(blob, ref.HEADER + 8 * (nblocks - 1), "<I", len(blob) // 8),
        "non-ascending offsets": _patched(_patched(blob, ref.HEADER + 8, "<I", int(at[2])),
                                          ref.HEADER + 16, "<I", int(at[1])),
        "k against bits": _patched(blob, ref.HEADER + 8 * mixed + 4, "<H", 5),
        "total": _patched(blob, 24, "<I", len(blob) - 8),
        "truncated": blob[:-8],
        "empty": b"",
    }


def test_validate_stream_agrees_with_the_pyref():
    for dtype in (np.uint32, np.uint64):
        vol = ref.class_volume(dtype=dtype)
        blob = ref.encode(vol)
        assert label_codec.validate_stream(blob, vol.dtype.itemsize, vol.shape) == vol.shape
        small = ref.encode(ref.class_volume((16, 16, 11), dtype, counts=(1, 3, 17, 512)))
        for name, bad in corruptions(small).items():
            with pytest.raises(ValueError):
                label_codec.validate_stream(bad, vol.dtype.itemsize, (16, 16, 11))
            if name != "empty":
                with pytest.raises(ValueError):
                    ref.validate(bad, vol.dtype.itemsize, (16, 16, 11))
        with pytest.raises(ValueError):
            label_codec.validate_stream(small, 12 - vol.dtype.itemsize)
        with pytest.raises(ValueError):
            label_codec.validate_stream(small, vol.dtype.itemsize, (16, 16, 12))


def test_a_corrupt_chunk_file_raises_before_any_device_call(tmp_path, monkeypatch):
    vol = ref.class_volume((16, 16, 11), np.uint64, counts=(1, 3, 17, 512))
    path = pyref_store(str(tmp_path / "labels"), vol, (16, 16, 16))
    victim = os.path.join(path, chunk_store.chunk_key(0, 0, 0))
    good = open(victim, "rb").read()
    calls = []

    def no_device(*a, **k):
        calls.append(a)
        raise AssertionError("a device call was attempted")

    monkeypatch.setattr(_native, "context", no_device)
    arr = chunk_store.open_zarr(path)
    for name, bad in corruptions(good).items():
        with open(victim, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            arr.read_patches([(4, 4, 4)], (6, 6, 6))
        assert arr.last_read is None, name
        with pytest.raises(ValueError):
            arr[0, 0, 1:3, 1:3, 1:3]
        with pytest.raises(ValueError):
            chunk_store.read_zarr(path)
        with pytest.raises(ValueError):
            chunk_store.read_chunk(path, 0, 0, 0)
    assert calls == []
    os.remove(victim)
    with pytest.raises(FileNotFoundError):
        arr.read_patches([(4, 4, 4)], (6, 6, 6))
    assert calls == []
    # the empty batch needs neither a file nor the device
    assert arr.read_patches(np.zeros((0, 3), np.int64), (6, 6, 6)).shape == (0, 6, 6, 6)
    # with the file back the read gets as far as the device
    with open(victim, "wb") as f:
        f.write(good)
    with pytest.raises(AssertionError):
        arr.read_patches([(4, 4, 4)], (6, 6, 6))
    assert len(calls) == 1
