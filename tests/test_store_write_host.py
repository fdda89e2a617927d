"""Host side of the region writes of a chunk store: the write planner against brute force, the
numpy restatement of the scatter entry against sequential numpy assignment, ``create_zarr`` / ``open_zarr(mode=)``,
and every check that is made before a device is touched.  No GPU."""
import json
import os

import numpy as np
import pytest

import region_pyref as ref
import region_write_pyref as wref
from aind_exaspim_image_compression.bm4d import denoise_store
from aind_exaspim_image_compression.utils import chunk_store, store_write
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec

BOX_A = (12, 10, 40)
STARTS_A = [(0, 0, 0), (4, 3, 10), (10, 10, 20), (-5, -4, -7), (30, 15, 50), (-40, 0, 0), (100, 100, 100),
            (4, 3, 10)]
BOX_B = (6, 9, 70)
STARTS_B = [(0, 0, 0), (3, 5, 30), (7, 7, 60), (-2, -3, -9), (15, 12, 100), (-30, 0, 0), (50, 50, 200), (3, 5, 30)]
GEOMETRIES = [(ref.SHAPE_A, ref.CHUNK_A, BOX_A, STARTS_A), (ref.SHAPE_B, ref.CHUNK_B, BOX_B, STARTS_B),
              ((37, 21, 70), (16, 16, 32), (16, 21, 38), [(0, 0, 0), (16, 0, 32), (32, 0, 0), (-3, 0, 64)])]


def _check_group(g, shape, chunk, starts, boxes, nominal, states):
    """One group against brute force; ``states``: what ``plan_ref`` says of the group's boxes."""
    got = {tuple(int(i) for i in idx): st for idx, st in zip(g.chunks, g.states)}
    assert got == states
    n_dec = sum(st == "decode" for st in g.states)
    assert g.states[:n_dec] == ["decode"] * n_dec                 # the chunks to decode come first ...
    dec_members = sorted(m for st in g.stacks[:g.decode_stacks] for m in st.members)
    assert dec_members == list(range(n_dec))                       # ... in stacks of their own
    assert sorted(m for st in g.stacks for m in st.members) == list(range(len(g.chunks)))
    assert len(g.stacks) <= 16
    # per chunk: exactly the boxes that touch it, ascending
    for m, idx in enumerate(g.chunks):
        want = [n - g.first for n in range(g.first, g.stop)
                if tuple(idx) in ref.touched_ref(shape, chunk, starts[n], boxes[n])]
        assert [int(k) for k in g.dst_boxes[m] if k >= 0] == want
    # the destinations: each chunk's extent, inside the pool, no two overlapping
    used = np.zeros(g.pool_elems, dtype=np.int32)
    for m, (idx, d) in enumerate(zip(g.chunks, g.dsts)):
        ext = tuple(min(c, s - int(i) * c) for i, c, s in zip(idx, chunk, shape))
        assert (d["z0"], d["y0"], d["x0"]) == tuple(int(i) * c for i, c in zip(idx, chunk))
        assert (d["ez"], d["ey"], d["ex"]) == ext
        z, y, x = (np.arange(e) for e in ext)
        used[int(d["base"]) + z[:, None, None] * int(d["stride_z"]) + y[None, :, None] * int(d["stride_y"]) +
             x[None, None, :]] += 1
    assert used.max(initial=0) <= 1
    for st in g.stacks:                                            # a stack is a volume of its members' chunks
        assert st.base % 128 == 0 and st.base + int(np.prod(st.shape)) <= g.pool_elems
        want_chunk = tuple(chunk) if nominal else tuple(min(c, v) for c, v in zip(chunk, st.shape))
        assert st.chunk == want_chunk
        assert int(np.prod([-(-v // c) for v, c in zip(st.shape, st.chunk)])) == len(st.members)


@pytest.mark.parametrize("geometry", range(len(GEOMETRIES)))
@pytest.mark.parametrize("nominal", [False, True])
def test_plan_write_against_brute_force(geometry, nominal):
    shape, chunk, box, starts = GEOMETRIES[geometry]
    boxes = [box] * len(starts)
    missing = {(0, 0, 0), (1, 0, 1), (0, 1, 2)}

    def exists(*idx):
        return tuple(idx) not in missing

    groups = store_write.plan_write(shape, chunk, starts, box, nominal, exists)
    assert len(groups) == 1 and (groups[0].first, groups[0].stop) == (0, len(starts))
    states = wref.plan_ref(shape, chunk, starts, boxes, exists)
    assert len(states) == len({t for s in starts for t in ref.touched_ref(shape, chunk, s, box)})
    _check_group(groups[0], shape, chunk, starts, boxes, nominal, states)
    if geometry == 2:                                              # slabs aligned to the grid or the array's edge
        assert set(states.values()) == {"covered", "decode", "zero"}
        assert states[(0, 0, 0)] == states[(1, 0, 1)] == states[(1, 1, 2)] == "covered"      # stored or not
        assert states[(0, 1, 2)] == "zero" and states[(0, 0, 1)] == "decode"
    else:
        assert {"decode", "zero"} <= set(states.values())
    # without `exists` every chunk is taken to be stored
    assert "zero" not in store_write.plan_write(shape, chunk, starts, box, nominal)[0].states


def test_plan_write_boxes_of_their_own_extents_and_outside():
    shape, chunk = (40, 24, 36), (8, 8, 16)
    starts = [(0, 0, 0), (16, 16, 32), (32, 0, 16), (-20, 0, 0), (40, 0, 0), (3, 3, 3)]
    boxes = [(16, 16, 16), (16, 8, 4), (8, 16, 16), (20, 8, 8), (4, 4, 4), (2, 30, 40)]
    (g,) = store_write.plan_write(shape, chunk, starts, boxes, False, lambda *idx: False)
    states = wref.plan_ref(shape, chunk, starts, boxes, lambda *idx: False)
    _check_group(g, shape, chunk, starts, boxes, False, states)
    assert states[(0, 0, 0)] == "covered" and states[(2, 2, 2)] == "covered" and states[(0, 2, 1)] == "zero"
    assert g.decode_stacks == 0
    # boxes wholly outside touch nothing; a plan of nothing is empty
    (g,) = store_write.plan_write(shape, chunk, [(-20, 0, 0), (40, 0, 0)], (20, 8, 8), False)
    assert len(g.chunks) == 0 and g.pool_elems == 0 and g.stacks == []
    assert store_write.plan_write(shape, chunk, np.zeros((0, 3), int), (4, 4, 4), False) == []
    with pytest.raises(ValueError):
        store_write.plan_write(shape, chunk, starts, (0, 4, 4), False)
    with pytest.raises(ValueError):
        store_write.plan_write(shape, chunk, starts, boxes[:3], False)


@pytest.mark.parametrize("cap", [1, 40000, 200000])
def test_plan_write_groups_under_a_cap(cap):
    shape, chunk, box, starts = GEOMETRIES[0]
    missing = {(0, 0, 0), (0, 0, 1)}

    def exists(*idx):
        return tuple(idx) not in missing

    groups = store_write.plan_write(shape, chunk, starts, box, False, exists, max_pool_bytes=cap)
    assert [g.first for g in groups] == [0] + [g.stop for g in groups[:-1]] and groups[-1].stop == len(starts)
    if cap == 1:
        assert len(groups) == len(starts)
    written = set()
    for g in groups:
        n = range(g.first, g.stop)
        # a chunk an earlier group wrote exists by the time this group runs
        states = wref.plan_ref(shape, chunk, [starts[i] for i in n], [box] * len(n),
                               lambda *idx: exists(*idx) or tuple(idx) in written)
        _check_group(g, shape, chunk, starts, [box] * len(starts), False, states)
        written.update(states)
        ids = {t for i in n for t in ref.touched_ref(shape, chunk, starts[i], box)}
        nbytes = sum(2 * int(np.prod([min(c, s - i * c) for i, c, s in zip(t, chunk, shape)])) for t in ids) + \
            sum(12 + 4 * len(ref.touched_ref(shape, chunk, starts[i], box)) for i in n)
        assert nbytes <= cap or len(n) == 1
    if cap == 200000:
        assert len(groups) == 1
    else:
        assert len(groups) > 1
        again = [g for g in groups[1:] if "decode" in g.states]
        assert again                                                # some chunk is read, changed and written twice


def test_scatter_boxes_ref_is_sequential_assignment():
    """Destinations that tile a volume, boxes that overlap each other: the restated entry equals ``for n: vol[box n]
    = v[n]``, and a box later in a list wins."""
    rng = np.random.default_rng(5)
    shape, chunk = (9, 10, 23), (4, 6, 8)
    vol = rng.integers(0, 65536, shape).astype(np.uint16)
    starts = [(1, 2, 3), (0, 0, 0), (3, 4, 9), (2, 3, 5), (-2, 6, 18), (20, 0, 0)]
    box = (5, 5, 9)
    values = rng.integers(0, 65536, (len(starts),) + box).astype(np.uint16)
    (g,) = store_write.plan_write(shape, chunk, starts, box, False)
    # lay the volume out in the plan's pool, scatter, read the pool back as a volume
    pool = np.full(g.pool_elems, 0xBEEF, dtype=np.uint16)

    def pool_index(d):
        z, y, x = (np.arange(d[k]) for k in ("ez", "ey", "ex"))
        return int(d["base"]) + z[:, None, None] * int(d["stride_z"]) + y[None, :, None] * int(d["stride_y"]) + \
            x[None, None, :]

    def region(d):
        return tuple(slice(int(d[o]), int(d[o]) + int(d[e])) for o, e in (("z0", "ez"), ("y0", "ey"), ("x0", "ex")))

    for d in g.dsts:
        pool[pool_index(d)] = vol[region(d)]
    got_pool = wref.scatter_boxes_ref(values, store_write.box_records(starts, box), pool, g.dsts, g.dst_boxes)
    got = vol.copy()                                               # the chunks no box touches are not in the pool
    assert len(g.dsts) < 18
    for d in g.dsts:
        got[region(d)] = got_pool[pool_index(d)]
    want = wref.assign_boxes(vol, starts, values)
    np.testing.assert_array_equal(got, want)
    assert np.any(want != vol) and np.any(want[3:5, 4:7, 9:12] == values[3][1:3, 1:4, 4:7])
    # the padding between stacks is not written
    touched = np.zeros(g.pool_elems, dtype=bool)
    for d in g.dsts:
        touched[pool_index(d)] = True
    assert np.all(got_pool[~touched] == 0xBEEF)
    # reversed lists: the first box wins instead
    rev = wref.scatter_boxes_ref(values, store_write.box_records(starts, box), pool, g.dsts, g.dst_boxes[:, ::-1])
    assert np.any(rev != got_pool)
    # float32 sources are added to, clipped and rounded to even; NaN gives 0
    v = np.array([-3, -0.5, 0.5, 1.5, 2.5, 65534.5, 65535.5, 7e4, np.inf, -np.inf, np.nan], dtype=np.float32)
    np.testing.assert_array_equal(wref.counts_ref(v, 0.0), [0, 0, 0, 2, 2, 65534, 65535, 65535, 65535, 0, 0])
    np.testing.assert_array_equal(wref.counts_ref(v, 31.7)[:5], [29, 31, 32, 33, 34])


def test_create_zarr_writes_the_metadata_only(tmp_path):
    path = str(tmp_path / "new")
    arr = chunk_store.create_zarr(path, ref.SHAPE_A, (1, 1) + ref.CHUNK_A, attributes={"who": "test"})
    assert os.listdir(path) == ["zarr.json"]
    with open(os.path.join(path, "zarr.json")) as f:
        assert json.load(f) == chunk_store.metadata(ref.SHAPE_A, ref.CHUNK_A, attributes={"who": "test"})
    assert arr.mode == "r+" and arr.shape == (1, 1) + ref.SHAPE_A and arr.chunks == (1, 1) + ref.CHUNK_A
    assert arr.last_write is None
    with pytest.raises(FileExistsError):
        chunk_store.create_zarr(path, ref.SHAPE_A, (1, 1) + ref.CHUNK_A)
    for codec in (BoundedDctCodec(4), BlockBoundedCodec(6, 0), ExacCodec(2, version=1)):
        arr = chunk_store.create_zarr(path, (1, 1) + ref.SHAPE_A, (1, 1) + ref.CHUNK_A, codec=codec, overwrite=True)
        with open(os.path.join(path, "zarr.json")) as f:
            assert json.load(f) == chunk_store.metadata(ref.SHAPE_A, ref.CHUNK_A, codec=codec)
        assert arr._write_codec is codec
    # an exac store states its chunk shape clamped to the array, the bounded formats keep the nominal one
    small = chunk_store.create_zarr(str(tmp_path / "small"), (10, 70, 20))
    assert small.chunks == (1, 1, 10, 64, 20)
    assert chunk_store.create_zarr(str(tmp_path / "small-b"), (10, 70, 20), codec=BoundedDctCodec(2)).chunks == \
        (1, 1, 64, 64, 64)
    with pytest.raises(ValueError):
        chunk_store.create_zarr(str(tmp_path / "bad"), (2, 1, 8, 8, 8))
    with pytest.raises(ValueError):
        chunk_store.create_zarr(str(tmp_path / "bad"), (8, 8, 8), chunks=(8, 8, 8))
    with pytest.raises(NotImplementedError):
        chunk_store.create_zarr(str(tmp_path / "bad"), (8, 8, 8), codec=ExacCodec(4))
    assert not os.path.exists(str(tmp_path / "bad"))


def test_open_zarr_modes_and_codecs(tmp_path):
    path = str(tmp_path / "s")
    chunk_store.create_zarr(path, ref.SHAPE_A, (1, 1) + ref.CHUNK_A, codec=ExacCodec(2, version=1))
    ro = chunk_store.open_zarr(path)
    assert ro.mode == "r"
    block = np.zeros((1, 1, 4, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="read-only"):
        ro[0, 0, 0:4, 0:4, 0:4] = block
    with pytest.raises(ValueError, match="read-only"):
        ro.write_patches([(0, 0, 0)], block[0], is_center=False)
    with pytest.raises(ValueError):
        chunk_store.open_zarr(path, mode="w")
    rw = chunk_store.open_zarr(path, mode="r+")
    assert rw.mode == "r+" and rw._write_codec.version == 1          # a write keeps the store's format version
    with pytest.raises(ValueError):
        chunk_store.open_zarr(path, mode="r+", codec=ExacCodec(2))    # version 2 is not what is stored
    with pytest.raises(ValueError):
        chunk_store.open_zarr(path, codec=BoundedDctCodec(4))
    # a bound table is not in the file: writing needs the codec that holds it, and only that one
    table = np.minimum(np.arange(65536) // 100, 6).astype(np.uint16)
    tab = BlockBoundedCodec(6, 0, bound_table=table)
    tpath = str(tmp_path / "t")
    chunk_store.create_zarr(tpath, ref.SHAPE_A, (1, 1) + ref.CHUNK_A, codec=tab)
    assert chunk_store.open_zarr(tpath).mode == "r"
    with pytest.raises(ValueError, match="codec="):
        chunk_store.open_zarr(tpath, mode="r+")
    assert chunk_store.open_zarr(tpath, mode="r+", codec=tab)._write_codec is tab
    with pytest.raises(ValueError):
        chunk_store.open_zarr(tpath, mode="r+", codec=BlockBoundedCodec(6, 0, bound_table=table + 1))
    with pytest.raises(ValueError):
        chunk_store.open_zarr(tpath, mode="r+", codec=BlockBoundedCodec(6, 0))
    # int32 stores: as on the read side
    ipath = str(tmp_path / "i")
    os.makedirs(ipath)
    with open(os.path.join(ipath, "zarr.json"), "w") as f:
        json.dump(chunk_store.metadata((8, 8, 8), (8, 8, 8), typesize=4), f)
    with pytest.raises(NotImplementedError):
        chunk_store.open_zarr(ipath, mode="r+")


def test_key_shape_and_value_errors_before_any_device(tmp_path):
    arr = chunk_store.create_zarr(str(tmp_path / "s"), ref.SHAPE_A, (1, 1) + ref.CHUNK_A)
    with pytest.raises(IndexError):
        arr[0, 0, ::2] = 0
    with pytest.raises(IndexError):
        arr[0, 0, 0, 0, 0, 0] = 0
    with pytest.raises(IndexError):
        arr[..., 0] = 0
    with pytest.raises(IndexError):
        arr[0, 0, 40] = 0
    with pytest.raises(ValueError):
        arr[0, 0, 0:4, 0:4, 0:4] = np.zeros((4, 4, 5), np.uint16)
    with pytest.raises(ValueError):
        arr[0, 0, 0:4, 0:4, 0:4] = np.zeros((1, 4, 4, 4), np.uint16)       # exactly the result shape
    with pytest.raises(ValueError):
        arr[0, 0, 0:4, 0:4, 0:4] = 65536
    with pytest.raises(ValueError):
        arr[0, 0, 0:4, 0:4, 0:4] = -1
    with pytest.raises(ValueError):
        arr[0, 0, 0:4, 0:4, 0:4] = np.zeros((4, 4, 4), np.complex64)
    patches = np.zeros((2, 4, 4, 4), np.uint16)
    for bad in (dict(voxels=[(0, 0, 0)]), dict(voxels=[(0.5, 0, 0), (0, 0, 0)]), dict(patches=patches[0]),
                dict(patches=patches.astype(np.float64)), dict(offset=3.0), dict(mask=np.ones(patches.shape, bool)),
                dict(voxels=[(2 ** 31, 0, 0), (0, 0, 0)])):
        kw = dict(dict(voxels=[(0, 0, 0), (8, 8, 8)], patches=patches), **bad)
        with pytest.raises(ValueError):
            arr.write_patches(kw.pop("voxels"), kw.pop("patches"), **kw)
        assert arr.last_write is None
    blk = chunk_store.create_zarr(str(tmp_path / "b"), ref.SHAPE_A, (1, 1) + ref.CHUNK_A, codec=BlockBoundedCodec(6, 0))
    with pytest.raises(ValueError):
        blk.write_patches([(0, 0, 0)], np.zeros((1, 16, 16, 32), np.uint16), is_center=False,
                          mask=np.ones((1, 16, 16, 31), bool))
    # nothing to write: no device, an empty report
    arr.write_patches(np.zeros((0, 3), int), np.zeros((0, 4, 4, 4), np.uint16))
    assert arr.last_write["chunks"] == 0 and arr.last_write["groups"] == 0
    arr[0, 0, 5:5, :, :] = 7
    assert arr.last_write["chunks"] == 0
    assert os.listdir(arr.path) == ["zarr.json"]


@pytest.mark.parametrize("codec", [BoundedDctCodec(4), BlockBoundedCodec(6, 0)])
def test_a_lossy_store_refuses_partial_chunks_from_the_plan_alone(tmp_path, codec):
    arr = chunk_store.create_zarr(str(tmp_path / "s"), ref.SHAPE_A, (1, 1) + ref.CHUNK_A, codec=codec)
    with pytest.raises(ValueError, match=r"chunk \(0, 0, 0\)"):
        arr[0, 0, 0:16, 0:16, 0:31] = 5
    with pytest.raises(ValueError, match=r"chunk \(2, 1, 2\)"):
        arr[0, 0, 32:37, 16:21, 65:70] = 5
    with pytest.raises(ValueError, match=r"chunk \(1, 0, 1\)"):                # the second box leaves the grid
        arr.write_patches([(0, 0, 0), (16, 0, 33)], np.zeros((2, 16, 16, 32), np.uint16), is_center=False)
    assert arr.last_write is None and os.listdir(arr.path) == ["zarr.json"]
    groups = store_write.plan_write(ref.SHAPE_A, ref.CHUNK_A, [(32, 16, 64), (0, 0, 0)], [(5, 5, 6), (16, 21, 64)],
                                    True, lambda *idx: False)
    store_write.check_lossy(arr, groups)                  # aligned to the grid and to the array's edge: fine


def test_denoise_store_checks_its_arguments_before_a_device(tmp_path):
    src = str(tmp_path / "src")
    chunk_store.create_zarr(src, (40, 24, 36), (1, 1, 16, 16, 32))
    dst = str(tmp_path / "dst")
    with pytest.raises(ValueError, match="multiple"):
        denoise_store(src, dst, 24.0, 37.0, chunk=24, halo=4)             # 24 is no multiple of 16 (nor of 32)
    with pytest.raises(ValueError, match="multiple"):
        denoise_store(src, dst, 24.0, 37.0, chunk=16, halo=4)             # the source's chunks are 32 wide
    with pytest.raises(ValueError, match="multiple"):
        denoise_store(src, dst, 24.0, 37.0, chunk=16, halo=4, chunks=(1, 1, 8, 8, 12))
    with pytest.raises(ValueError, match="auto"):
        denoise_store(src, dst, "auto", 37.0, chunk=32, halo=4)
    with pytest.raises(ValueError, match="auto"):
        denoise_store(src, dst, noise="auto", chunk=32, halo=4)
    with pytest.raises(ValueError):
        denoise_store(src, dst, chunk=32, halo=4)                          # neither sigma nor noise
    with pytest.raises(ValueError):
        denoise_store(src, dst, 24.0, noise={"gain": 2.0, "read_noise": 3.0, "offset": 37.0}, chunk=32)
    with pytest.raises(ValueError, match="thinner"):
        denoise_store(src, dst, 24.0, 37.0, chunk=33, halo=0, chunks=(1, 1, 33, 33, 33))       # 40 = 33 + 7
    with pytest.raises(ValueError):
        denoise_store(src, dst, 24.0, 37.0, chunk=32, halo=65)
    with pytest.raises(ValueError):
        denoise_store(src, dst, 24.0, 37.0, chunk=32, halo=4, stages=3)
    with pytest.raises(ValueError):
        denoise_store(src, dst, 24.0, 37.0, chunk=32, halo=4, budget_bytes=0)
    with pytest.raises(ValueError):
        denoise_store(src, dst, 24.0, 37.0, chunk=32, halo=4, chunks=(16, 16, 32))
    assert not os.path.exists(dst)
