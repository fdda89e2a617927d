"""Out-of-core component labelling on the GPU: ``components_store`` / ``components_volume`` against the
in-memory labeller and the canonicalised scipy labels, byte for byte against ``write_zarr`` of the expectation, under
two brick plans; the two entries on their own; the produced store read back by patches.  Exact equality everywhere."""
import os

import numpy as np
import pytest

import segment_pyref
from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import chunk_store, store_segment
from aind_exaspim_image_compression.utils.label_codec import LabelCodec

pytestmark = pytest.mark.gpu

SHAPE = (20, 24, 70)
CHUNKS = (1, 1, 8, 8, 32)          # 3 x 3 x 3 chunks, the last of each axis partial; x crosses the labeller's 64-wide tile
ONE_CHUNK_BRICKS = 1               # budget_bytes under which every brick is a single chunk


def _random(density):
    return lambda: np.random.default_rng(int(1000 * density)).random(SHAPE) < density


def _serpentine():
    """One voxel wide, one component under 6 and 26: every second row of every second plane, joined at alternating
    ends -- through every brick many times, so the merge sees a long chain."""
    m = np.zeros(SHAPE, dtype=bool)
    flip = False
    for z in range(0, SHAPE[0], 2):
        rows = list(range(0, SHAPE[1], 2))
        rows = rows[::-1] if (z // 2) % 2 else rows
        for i, y in enumerate(rows):
            m[z, y, :] = True
            if i + 1 < len(rows):
                m[z, (y + rows[i + 1]) // 2, -1 if flip else 0] = True
                flip = not flip
        if z + 2 < SHAPE[0]:
            m[z + 1, rows[-1], 0 if flip else -1] = True     # (the end at which the last row of the plane stopped)
    return m


def _diagonals():
    """Voxels joined only through corners, across one, two and three brick faces at a time."""
    m = np.zeros(SHAPE, dtype=bool)
    i = np.arange(20)
    m[i, i, i] = True
    m[i, i, 24 + i] = True                                   # (7, 7, 31) -> (8, 8, 32): the corner of eight bricks
    m[i, i + 2, 45 + i] = True
    return m


def _checkerboard():
    z, y, x = np.indices(SHAPE)
    return (z + y + x) % 2 == 0


def _halo_only():
    """Components that a brick sees in its halo alone: the first voxels past brick (0, 0, 0) on one, two and three
    axes, and one voxel of that brick which touches the corner one under 26-connectivity."""
    m = np.zeros(SHAPE, dtype=bool)
    for v in ((8, 3, 5), (3, 8, 5), (3, 3, 32), (8, 8, 5), (8, 8, 32), (7, 7, 31), (16, 16, 64), (19, 23, 69)):
        m[v] = True
    return m


INPUTS = {"random_005": _random(0.05), "random_03": _random(0.3), "random_06": _random(0.6),
          "serpentine": _serpentine, "diagonals": _diagonals, "checkerboard": _checkerboard,
          "empty": lambda: np.zeros(SHAPE, dtype=bool), "full": lambda: np.ones(SHAPE, dtype=bool),
          "halo_only": _halo_only}
_cache = {}


def _expected(name, connectivity):
    """(mask, whole-volume labels uint64): computed once, shared, never changed."""
    key = (name, connectivity)
    if key not in _cache:
        mask = INPUTS[name]()
        want = segment_pyref.first_voxel_labels(mask, connectivity)
        mask.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (mask, want)
    return _cache[key]


def _source(tmp_path, mask):
    src = str(tmp_path / "src.zarr")
    chunk_store.write_zarr((mask.astype(np.uint16) * 700 + 30), src, chunks=CHUNKS)
    return src


def _chunk_files(path):
    found = {}
    for root, _, files in os.walk(os.path.join(path, "c")):
        for f in files:
            full = os.path.join(root, f)
            with open(full, "rb") as fh:
                found[os.path.relpath(full, path)] = fh.read()
    return found


def _check_table(res, want):
    ids, counts = np.unique(want[want != 0], return_counts=True)
    assert res["n_components"] == ids.size and res["n_kept_components"] == ids.size
    assert res["n"] == want.size and res["n_seed"] == int(np.count_nonzero(want)) == res["n_kept_voxels"]
    assert res["largest"] == (int(counts.max()) if counts.size else 0)
    assert res["labels"].dtype == np.uint64 and res["sizes"].dtype == np.uint64
    np.testing.assert_array_equal(res["labels"], ids)
    np.testing.assert_array_equal(res["sizes"], np.bincount(want.reshape(-1).astype(np.int64))[ids.astype(np.int64)])


# ---- the store path, every input, both brick plans -----------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_components_store_is_whole_volume_labelling(tmp_path, name, connectivity):
    mask, want = _expected(name, connectivity)
    in_memory, n = metrics.label_components(mask, connectivity)
    np.testing.assert_array_equal(in_memory.view(np.uint32), want)             # the two references agree
    src = _source(tmp_path, mask)
    ref = str(tmp_path / "ref.zarr")
    chunk_store.write_zarr(want.astype(np.uint32), ref, chunks=CHUNKS, codec=LabelCodec(4))
    ref_files = _chunk_files(ref)
    assert len(ref_files) == 27
    for tag, budget, bricks in (("chunks", ONE_CHUNK_BRICKS, 27), ("whole", 4 << 30, 1)):
        dst = str(tmp_path / ("dst_%s.zarr" % tag))
        stats = {}
        res = metrics.components_store(src, dst, threshold=100, connectivity=connectivity, budget_bytes=budget,
                                       stats=stats)
        assert stats["bricks"] == bricks and stats["passes"] == 2 and res["cut"] == 101
        got = chunk_store.open_zarr(dst)
        assert got.dtype == np.uint32 and tuple(got.chunks) == CHUNKS
        np.testing.assert_array_equal(got[0, 0], want)
        assert _chunk_files(dst) == ref_files                                  # chunk file for chunk file, both plans
        assert res["n_components"] == n
        _check_table(res, want)
        assert set(stats["seconds"]) == {"measure", "read", "label", "collect", "merge", "relabel", "encode",
                                         "files_write"}
        assert stats["records"]["size"] >= n and 0 <= stats["collect_repeats"] <= bricks
        if bricks == 1:
            assert stats["records"]["halo"] == stats["records"]["face"] == 0


def test_the_serpentine_is_one_component_and_the_diagonals_split_at_6():
    for name, connectivity, n in (("serpentine", 6, 1), ("serpentine", 26, 1), ("diagonals", 26, 3),
                                  ("diagonals", 6, 60), ("checkerboard", 26, 1)):
        want = _expected(name, connectivity)[1]
        assert np.unique(want[want != 0]).size == n


# ---- min_voxels past the old cap, relabel, the two label types ------------------------------------------------------
@pytest.mark.parametrize("min_voxels", [2, 65, 1000])
def test_min_voxels_has_no_cap(tmp_path, min_voxels):
    mask, whole = _expected("random_03", 6)
    want, labels, sizes = segment_pyref.whole_volume(mask, 6, min_voxels)
    src = _source(tmp_path, mask)
    dst = str(tmp_path / "dst.zarr")
    res = metrics.components_store(src, dst, threshold=100, connectivity=6, min_voxels=min_voxels,
                                   budget_bytes=ONE_CHUNK_BRICKS)
    np.testing.assert_array_equal(chunk_store.open_zarr(dst)[0, 0], want)
    np.testing.assert_array_equal(res["labels"], labels)
    np.testing.assert_array_equal(res["sizes"], sizes)
    assert res["n_components"] == np.unique(whole[whole != 0]).size
    assert res["n_kept_components"] == labels.size and res["n_kept_voxels"] == int(sizes.sum())
    assert res["n_seed"] == int(np.count_nonzero(mask))
    ref = str(tmp_path / "ref.zarr")
    chunk_store.write_zarr(want.astype(np.uint32), ref, chunks=CHUNKS, codec=LabelCodec(4))
    assert _chunk_files(dst) == _chunk_files(ref)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_relabel_is_scipys_numbering(tmp_path, connectivity):
    mask, _ = _expected("random_03", connectivity)
    want, n = metrics.label_components(mask, connectivity, relabel=True)
    dst = str(tmp_path / "dst.zarr")
    res = metrics.components_store(_source(tmp_path, mask), dst, threshold=100, connectivity=connectivity, relabel=True,
                                   budget_bytes=ONE_CHUNK_BRICKS)
    np.testing.assert_array_equal(chunk_store.open_zarr(dst)[0, 0], want.astype(np.uint32))
    np.testing.assert_array_equal(res["labels"], np.arange(1, n + 1, dtype=np.uint64))
    vol, _ = metrics.components_volume(mask, connectivity=connectivity, relabel=True, min_voxels=3, brick=(8, 8, 32))
    np.testing.assert_array_equal(vol, segment_pyref.whole_volume(mask, connectivity, 3, True)[0])


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_both_label_types(tmp_path, dtype):
    mask, want = _expected("random_03", 26)
    dst, ref = str(tmp_path / "dst.zarr"), str(tmp_path / "ref.zarr")
    res = metrics.components_store(_source(tmp_path, mask), dst, threshold=100, dtype=dtype,
                                   budget_bytes=ONE_CHUNK_BRICKS, attributes={"made_by": "test"})
    got = chunk_store.open_zarr(dst)
    assert got.dtype == np.dtype(dtype) and got.meta["attributes"]["made_by"] == "test"
    np.testing.assert_array_equal(got[0, 0], want.astype(dtype))
    chunk_store.write_zarr(want.astype(dtype), ref, chunks=CHUNKS, codec=LabelCodec(np.dtype(dtype).itemsize))
    assert _chunk_files(dst) == _chunk_files(ref)
    written = sum(len(b) for b in _chunk_files(dst).values())
    assert res["cratio"] == np.dtype(dtype).itemsize * mask.size / written


def test_other_destination_chunks_and_a_measured_cut(tmp_path):
    mask, want = _expected("random_005", 26)
    src = _source(tmp_path, mask)
    dst, ref = str(tmp_path / "dst.zarr"), str(tmp_path / "ref.zarr")
    stats = {}
    res = metrics.components_store(src, dst, k=6.0, chunks=(1, 1, 16, 8, 24), budget_bytes=ONE_CHUNK_BRICKS, stats=stats)
    assert stats["passes"] == 3 and 30 < res["cut"] <= 730                     # the seeds are the voxels at 730
    np.testing.assert_array_equal(chunk_store.open_zarr(dst)[0, 0], want)
    chunk_store.write_zarr(want.astype(np.uint32), ref, chunks=(1, 1, 16, 8, 24), codec=LabelCodec(4))
    assert _chunk_files(dst) == _chunk_files(ref)


# ---- the in-memory twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", ["random_03", "serpentine", "halo_only"])
def test_components_volume_does_not_depend_on_the_bricks(name, connectivity):
    mask, want = _expected(name, connectivity)
    one, table_one = metrics.components_volume(mask, connectivity=connectivity)
    stats = {}
    many, table_many = metrics.components_volume(mask, connectivity=connectivity, brick=(8, 8, 32), stats=stats)
    assert stats["bricks"] == 27 and one.dtype == np.uint32
    np.testing.assert_array_equal(one, want)
    np.testing.assert_array_equal(many, one)
    for key in table_one:
        np.testing.assert_array_equal(table_one[key], table_many[key])
    _check_table(table_many, want)
    odd, _ = metrics.components_volume(mask.view(np.uint8), connectivity=connectivity, brick=(7, 5, 13),
                                       dtype=np.uint64)
    np.testing.assert_array_equal(odd, want)
    counts = (mask.astype(np.uint16) * 700 + 30)
    as_volume, table = metrics.components_volume(counts, threshold=100, connectivity=connectivity, brick=(8, 8, 32))
    np.testing.assert_array_equal(as_volume, want)
    assert table["cut"] == 101


def test_the_driver_repeats_a_collection_whose_size_records_overflow(monkeypatch):
    mask, want = _expected("random_03", 6)
    monkeypatch.setattr(store_segment, "SIZE_RECORDS_MIN", 1)
    monkeypatch.setattr(store_segment, "SIZE_RECORDS_DIV", 1 << 62)
    stats = {}
    got, table = metrics.components_volume(mask, connectivity=6, brick=(8, 8, 32), stats=stats)
    assert stats["collect_repeats"] >= 1
    np.testing.assert_array_equal(got, want)
    _check_table(table, want)


# ---- the entries on their own ---------------------------------------------------------------------------------------
W0, WD = (3, 5, 7), (13, 12, 41)          # a window inside the volume, at an odd x
B0, BD = (4, 5, 10), (9, 11, 35)          # a brick inside it: low faces on z and x that are not the window's


def _window_labels(ctx, mask, connectivity):
    """uint32 labels of the window W0 + WD as ``component_seeds_u16`` (region = window) makes them, on the device."""
    sub = np.ascontiguousarray(mask[tuple(slice(o, o + d) for o, d in zip(W0, WD))]).view(np.uint8)
    d_labels = ctx.alloc(4 * sub.size)
    with ctx.to_device(sub) as d_sub:
        ctx.label_components(d_sub, np.uint8, WD, connectivity=connectivity, labels=d_labels)
        ctx.sync()
    return d_labels, sub.view(bool)


def _entry_expectation(mask, connectivity):
    sub = mask[tuple(slice(o, o + d) for o, d in zip(W0, WD))]
    prov = segment_pyref.provisional(segment_pyref.first_voxel_labels(sub, connectivity), SHAPE, W0, WD)
    zz, yy, xx = np.meshgrid(*[np.arange(o, o + w) for o, w in zip(W0, WD)], indexing="ij")
    vox = ((zz * SHAPE[1] + yy) * SHAPE[2] + xx).astype(np.uint64)
    inside = np.ones(WD, dtype=bool)
    low = np.zeros(WD, dtype=bool)
    for a, c in enumerate((zz, yy, xx)):
        inside &= (c >= B0[a]) & (c < B0[a] + BD[a])
        low |= (c == B0[a]) & (B0[a] > 0)
    seed = prov != 0
    rec = lambda sel: segment_pyref._sorted(np.stack([vox[sel], prov[sel]], axis=1))     # noqa: E731
    ids, own = np.unique(prov[seed & inside], return_counts=True)
    crop = tuple(slice(b - w, b - w + d) for b, w, d in zip(B0, W0, BD))
    return prov, rec(seed & ~inside), rec(seed & inside & low), np.stack([ids, own.astype(np.uint64)], axis=1), crop


@pytest.mark.parametrize("connectivity", [6, 26])
def test_collect_entry(ctx, connectivity):
    mask, _ = _expected("random_03", connectivity)
    prov, halo, face, size, _ = _entry_expectation(mask, connectivity)
    halo_cap, face_cap = _native.segment_record_capacities(WD, B0, BD)
    assert halo_cap == np.prod(WD) - np.prod(BD) and face_cap == np.prod(BD) - 8 * 10 * 34
    d_labels, _ = _window_labels(ctx, mask, connectivity)
    with d_labels, ctx.alloc(4 * int(np.prod(WD))) as d_own, ctx.alloc(16 * halo_cap) as d_halo, \
            ctx.alloc(16 * face_cap) as d_face, ctx.alloc(16 * len(size)) as d_size, ctx.alloc(24) as d_counts:
        geometry = (SHAPE, W0, WD, B0, BD)
        # a capacity of one: every record is counted, one is stored
        d_size.fill(0xFF)
        ctx.segment_collect(d_labels, *geometry, d_own, d_halo, halo_cap, d_face, face_cap, d_size, 1, d_counts)
        counts = d_counts.download((3,), np.uint64)
        np.testing.assert_array_equal(counts, [len(halo), len(face), len(size)])
        stored = d_size.download((len(size), 2), np.uint64)
        assert np.all(stored[1:] == np.uint64(2 ** 64 - 1))                    # nothing past the capacity
        assert np.any(np.all(size == stored[0], axis=1))
        # room for all
        ctx.segment_collect(d_labels, *geometry, d_own, d_halo, halo_cap, d_face, face_cap, d_size, len(size), d_counts)
        np.testing.assert_array_equal(d_counts.download((3,), np.uint64), counts)
        np.testing.assert_array_equal(segment_pyref._sorted(d_halo.download((len(halo), 2), np.uint64)), halo)
        np.testing.assert_array_equal(segment_pyref._sorted(d_face.download((len(face), 2), np.uint64)), face)
        np.testing.assert_array_equal(segment_pyref._sorted(d_size.download((len(size), 2), np.uint64)), size)
        own = d_own.download((int(np.prod(WD)),), np.uint32)
        roots = np.flatnonzero(own)
        assert int(own.sum()) == int(size[:, 1].sum()) and roots.size == len(size)
        # the arguments are checked on the host
        for bad in ((d_halo, halo_cap - 1, d_face, face_cap, d_size, 4), (d_halo, halo_cap, d_face, face_cap - 1, d_size, 4),
                    (d_halo, halo_cap, d_face, face_cap, d_size, 0), (None, halo_cap, d_face, face_cap, d_size, 4),
                    (int(d_halo.ptr) + 8, halo_cap, d_face, face_cap, d_size, 4)):
            with pytest.raises(ValueError):
                ctx.segment_collect(d_labels, *geometry, d_own, *bad, d_counts)
        with pytest.raises(ValueError):                                       # the window leaves the volume
            ctx.segment_collect(d_labels, SHAPE, W0, (13, 12, 64), B0, BD, d_own, d_halo, 1 << 20, d_face, 1 << 20,
                                d_size, 4, d_counts)


@pytest.mark.parametrize("typesize", [4, 8])
def test_relabel_entry(ctx, typesize):
    mask, _ = _expected("random_03", 6)
    prov, _, _, size, crop = _entry_expectation(mask, 6)
    assert len(size) > 100
    dtype = np.uint32 if typesize == 4 else np.uint64
    nvox = int(np.prod(BD))
    d_labels, _ = _window_labels(ctx, mask, 6)
    with d_labels, ctx.alloc(typesize * int(np.prod(WD))) as d_final, ctx.alloc(typesize * nvox + 16) as d_out:
        geometry = (SHAPE, W0, WD, B0, BD)
        # an empty table: the provisional labels (the window begins at x = 7, the brick at x = 10: rows of the labels
        # start at every alignment; 35 voxels a row of the output, so do the stores)
        ctx.segment_relabel(d_labels, *geometry, None, None, 0, typesize, d_final, d_out)
        np.testing.assert_array_equal(d_out.download(BD, dtype), prov[crop].astype(dtype))
        # a table that renames every second component, drops every fifth and does not know the others
        keys = size[::2, 0].copy()
        vals = np.arange(1, keys.size + 1, dtype=np.uint64) * 3
        vals[::5] = 0
        if typesize == 8:
            vals[1::5] += np.uint64(2 ** 40)
        table = dict(zip(keys.tolist(), vals.tolist()))
        want = np.vectorize(lambda p: table.get(int(p), int(p)), otypes=[np.uint64])(prov[crop])
        with ctx.to_device(keys) as d_keys, ctx.to_device(vals) as d_vals:
            ctx.segment_relabel(d_labels, *geometry, d_keys, d_vals, keys.size, typesize, d_final, d_out)
            np.testing.assert_array_equal(d_out.download(BD, dtype), want.astype(dtype))
            # an output that is not 16-byte aligned
            ctx.segment_relabel(d_labels, *geometry, d_keys, d_vals, keys.size, typesize, d_final,
                                int(d_out.ptr) + typesize)
            shifted = d_out.download((nvox + 1,), dtype)[1:].reshape(BD)
            np.testing.assert_array_equal(shifted, want.astype(dtype))
            for bad in ((d_keys, d_vals, keys.size, 2), (None, d_vals, keys.size, typesize),
                        (int(d_keys.ptr) + 4, d_vals, keys.size, typesize)):
                with pytest.raises(ValueError):
                    ctx.segment_relabel(d_labels, *geometry, *bad, d_final, d_out)
        with pytest.raises(ValueError):                                       # the brick leaves the window
            ctx.segment_relabel(d_labels, SHAPE, W0, WD, B0, (9, 13, 35), None, None, 0, typesize, d_final, d_out)


# ---- downstream -----------------------------------------------------------------------------------------------------
def test_the_produced_store_is_read_by_patches(tmp_path):
    mask, want = _expected("random_03", 26)
    dst = str(tmp_path / "dst.zarr")
    metrics.components_store(_source(tmp_path, mask), dst, threshold=100, budget_bytes=ONE_CHUNK_BRICKS)
    arr = chunk_store.open_zarr(dst)
    voxels = np.array([[0, 0, 0], [10, 12, 35], [19, 23, 69], [8, 8, 32], [3, 20, 64]])
    box = (6, 7, 9)
    got = arr.read_patches(voxels, box)
    padded = np.pad(want, [(b, b) for b in box])
    for n, v in enumerate(voxels):
        start = [int(c) - b // 2 + b for c, b in zip(v, box)]
        crop = padded[tuple(slice(s, s + b) for s, b in zip(start, box))]
        np.testing.assert_array_equal(got[n], crop.astype(np.uint32))
