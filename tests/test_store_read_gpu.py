"""Region reads of a chunk store on the MI355X: ``open_zarr(...).read_patches`` / ``[...]`` and
``Context.gather_boxes`` against numpy slicing of what the stores hold -- the original array for ``exac`` stores, the
reconstruction the bounded formats' Python references return for the lossy ones.  The stores are built on the host
(``region_pyref.build_stores``), once per module.  Every comparison is ``array_equal``."""
import os
import shutil

import numpy as np
import pytest

import region_pyref as ref
from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store

pytestmark = pytest.mark.gpu

BOX_A = (12, 10, 40)
STARTS_A = [(0, 0, 0), (4, 3, 10), (10, 10, 20), (-5, -4, -7), (30, 15, 50), (-40, 0, 0), (100, 100, 100),
            (4, 3, 10)]
BOX_B = (6, 9, 70)          # crosses both 64-wide chunks of a row and reaches the 8-wide one
STARTS_B = [(0, 0, 0), (3, 5, 30), (7, 7, 60), (-2, -3, -9), (15, 12, 100), (-30, 0, 0), (50, 50, 200), (3, 5, 30)]
NAMES_A = ["A-exac2", "A-exac1", "A-dctq", "A-block"]
NAMES_B = ["B-exac2", "B-dctq"]


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    return ref.build_stores(tmp_path_factory.mktemp("stores"))


def _geometry(name):
    return (ref.SHAPE_A, ref.CHUNK_A, BOX_A, STARTS_A) if name[0] == "A" else (ref.SHAPE_B, ref.CHUNK_B, BOX_B, STARTS_B)


def test_fixture_stores_hold_both_modes(stores):
    for name in ("A-dctq", "A-block", "B-dctq"):
        modes = {blob[3] for blob in stores[name][2]}
        assert modes == {0, 1}, (name, modes)
    assert len(stores["A-exac2"][2]) == 18
    assert {blob[2] for blob in stores["A-exac1"][2]} == {1} and {blob[2] for blob in stores["A-exac2"][2]} == {2}


@pytest.mark.parametrize("name", NAMES_A + NAMES_B)
def test_read_patches(stores, name):
    path, expected, _ = stores[name]
    shape, chunk, box, starts = _geometry(name)
    arr = chunk_store.open_zarr(path)
    assert arr.shape == (1, 1) + shape and arr.chunks == (1, 1) + chunk and arr.ndim == 5 and arr.dtype == np.uint16
    got = arr.read_patches(starts, box, is_center=False, fill=9)
    assert got.dtype == np.uint16 and got.shape == (len(starts),) + box
    np.testing.assert_array_equal(got, ref.slice_boxes(expected, starts, box, fill=9))
    assert np.all(got[5] == 9) and np.all(got[6] == 9)                    # wholly outside
    want_chunks = len({t for s in starts for t in ref.touched_ref(shape, chunk, s, box)})
    assert arr.last_read["chunks"] == want_chunks and arr.last_read["groups"] == 1
    assert arr.last_read["decode_calls"] <= 8
    # centred boxes: start = voxel - d // 2
    centres = [tuple(s + d // 2 for s, d in zip(st, box)) for st in starts]
    np.testing.assert_array_equal(arr.read_patches(centres, box, fill=9), got)
    # one voxel, the whole array, and a box around the array that touches every chunk
    np.testing.assert_array_equal(arr.read_patches([(5, 6, 33), (-1, 0, 0)], (1, 1, 1), is_center=False, fill=3),
                                  np.array([expected[5, 6, 33], 3], np.uint16).reshape(2, 1, 1, 1))
    np.testing.assert_array_equal(arr.read_patches([(0, 0, 0)], shape, is_center=False)[0], expected)
    big, org = (48, 32, 96) if name[0] == "A" else (28, 27, 146), (-3, -2, -5)
    np.testing.assert_array_equal(arr.read_patches([org], big, is_center=False),
                                  ref.slice_boxes(expected, [org], big))
    assert arr.last_read["chunks"] == int(np.prod([-(-s // c) for s, c in zip(shape, chunk)]))
    assert arr.read_patches(np.zeros((0, 3), int), box).shape == (0,) + box


@pytest.mark.parametrize("name", ["A-exac2", "A-block", "B-dctq"])
def test_read_patches_float32_with_offset(stores, name):
    path, expected, _ = stores[name]
    _, _, box, starts = _geometry(name)
    arr = chunk_store.open_zarr(path)
    got = arr.read_patches(starts, box, is_center=False, dtype=np.float32, offset=31.7, fill=-1.0)
    inside = ref.slice_boxes(np.ones_like(expected), starts, box, fill=0).astype(bool)
    want = ref.slice_boxes(expected, starts, box).astype(np.float32) - np.float32(31.7)
    want[~inside] = np.float32(-1.0)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        arr.read_patches(starts, box, dtype=np.uint16, offset=31.7)
    with pytest.raises(ValueError):
        arr.read_patches(starts, box, dtype=np.float64)


@pytest.mark.parametrize("name", ["A-exac2", "A-dctq"])
def test_getitem(stores, name):
    path, expected, _ = stores[name]
    arr = chunk_store.open_zarr(path)
    e5 = expected[np.newaxis, np.newaxis]
    np.testing.assert_array_equal(arr[0, 0, 3:30, :, 65:], e5[0, 0, 3:30, :, 65:])
    np.testing.assert_array_equal(arr[0, 0, -6:, 2, :-1], e5[0, 0, -6:, 2, :-1])
    whole = arr[:]
    assert whole.shape == e5.shape and whole.dtype == np.uint16
    np.testing.assert_array_equal(whole, chunk_store.read_zarr(path))
    np.testing.assert_array_equal(whole, e5)
    empty = arr[0, 0, 5:5, :, 3:]
    assert empty.shape == (0, 21, 67) and empty.dtype == np.uint16
    with pytest.raises(IndexError):
        arr[0, 0, ::2]
    # the reference's call sites
    from aind_exaspim_image_compression.utils.img_util import get_patch, get_slices
    s = get_slices((20, 10, 35), (8, 8, 16))
    np.testing.assert_array_equal(arr[(0, 0, *s)], e5[(0, 0, *s)])
    np.testing.assert_array_equal(get_patch(arr, (20, 10, 35), (8, 8, 16)), get_patch(e5, (20, 10, 35), (8, 8, 16)))


def test_only_touched_chunks_are_read(stores, tmp_path):
    path, expected, _ = stores["A-exac2"]
    copy = str(tmp_path / "pruned")
    shutil.copytree(path, copy)
    start = (4, 3, 10)
    touched = ref.touched_ref(ref.SHAPE_A, ref.CHUNK_A, start, BOX_A)
    grid = [-(-s // c) for s, c in zip(ref.SHAPE_A, ref.CHUNK_A)]
    for iz in range(grid[0]):
        for iy in range(grid[1]):
            for ix in range(grid[2]):
                if (iz, iy, ix) not in touched:
                    os.remove(os.path.join(copy, chunk_store.chunk_key(iz, iy, ix)))
    arr = chunk_store.open_zarr(copy)
    np.testing.assert_array_equal(arr.read_patches([start], BOX_A, is_center=False),
                                  ref.slice_boxes(expected, [start], BOX_A))
    assert arr.last_read["chunks"] == len(touched) == 2
    assert arr.last_read["chunk_bytes"] == sum(os.path.getsize(os.path.join(copy, chunk_store.chunk_key(*t)))
                                               for t in touched)
    os.remove(os.path.join(copy, chunk_store.chunk_key(*touched[-1])))
    with pytest.raises(FileNotFoundError):
        arr.read_patches([start], BOX_A, is_center=False)


@pytest.mark.parametrize("name", ["A-exac2", "A-block", "B-dctq"])
def test_memory_cap_does_not_change_results(stores, name):
    path, expected, _ = stores[name]
    _, _, box, starts = _geometry(name)
    capped = chunk_store.open_zarr(path, max_pool_bytes=1)
    got = capped.read_patches(starts, box, is_center=False, fill=9)
    assert capped.last_read["groups"] == len(starts)
    np.testing.assert_array_equal(got, chunk_store.open_zarr(path).read_patches(starts, box, is_center=False, fill=9))
    np.testing.assert_array_equal(got, ref.slice_boxes(expected, starts, box, fill=9))


@pytest.mark.parametrize("name", NAMES_A)
def test_a_corrupt_chunk_raises_and_the_context_stays_usable(stores, tmp_path, name):
    path, expected, _ = stores[name]
    copy = str(tmp_path / "corrupt")
    shutil.copytree(path, copy)
    start = (4, 3, 10)
    victim = os.path.join(copy, chunk_store.chunk_key(*ref.touched_ref(ref.SHAPE_A, ref.CHUNK_A, start, BOX_A)[1]))
    blob = bytearray(open(victim, "rb").read())
    blob[0] ^= 0xFF
    with open(victim, "wb") as f:
        f.write(bytes(blob))
    with pytest.raises(ValueError):
        chunk_store.open_zarr(copy).read_patches([start], BOX_A, is_center=False)
    np.testing.assert_array_equal(chunk_store.open_zarr(path).read_patches([start], BOX_A, is_center=False),
                                  ref.slice_boxes(expected, [start], BOX_A))


def _src_table(rows):
    t = np.zeros(len(rows), dtype=_native.BOX_SRC)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def test_gather_boxes_on_a_synthetic_pool(ctx):
    rng = np.random.default_rng(23)
    pool = rng.integers(0, 65536, 4001).astype(np.uint16)
    # (base, stride_y, stride_z, z0, y0, x0, ez, ey, ex): two overlapping sources with their own strides, one apart
    srcs = _src_table([(3, 17, 17 * 6, 0, 0, 0, 4, 6, 17), (1001, 40, 40 * 9, 2, 1, 5, 5, 9, 33),
                       (3000, 9, 9 * 3, 0, 0, 40, 3, 3, 9)])
    box, starts = (7, 8, 51), np.array([[-1, -1, -2], [0, 0, 0], [2, 1, 5], [3, 2, 11]], dtype=np.int32)
    lists = np.array([[0, 1, 2], [1, 0, 2], [2, -1, 1], [-1, -1, -1]], dtype=np.int32)
    n_out = len(starts) * int(np.prod(box))
    guard = 64

    def run(pool_dev, out_dtype, **kw):
        item = np.dtype(out_dtype).itemsize
        d_out = ctx.alloc(n_out * item + 2 * guard).fill(0xA5)
        try:
            ctx.gather_boxes(pool_dev, len(pool), kw.pop("srcs", srcs), kw.pop("lists", lists), starts, box,
                             int(d_out.ptr) + guard, out_dtype, **kw)
            ctx.sync()
        finally:
            raw = d_out.download((n_out * item + 2 * guard,), np.uint8)
            d_out.free()
        assert np.all(raw[:guard] == 0xA5) and np.all(raw[-guard:] == 0xA5)
        return raw[guard:-guard].view(out_dtype).reshape((len(starts),) + box), raw

    d_pool = ctx.to_device(pool)
    d_odd = ctx.to_device(np.concatenate([np.array([0xBEEF], np.uint16), pool, np.array([0xBEEF], np.uint16)]))
    try:
        want = ref.gather_boxes_ref(pool, srcs, lists, starts, box, fill=77)
        got, _ = run(d_pool, np.uint16, fill=77)
        np.testing.assert_array_equal(got, want)
        assert np.any(got[0] != got[1]) and np.all(got[3] == 77)          # the order of a list matters; no source
        # the pool at an odd element of a larger buffer: 2-byte alignment is enough
        got_odd, _ = run(int(d_odd.ptr) + 2, np.uint16, fill=77)
        np.testing.assert_array_equal(got_odd, want)
        want_f = ref.gather_boxes_ref(pool, srcs, lists, starts, box, np.float32, 31.7, -1.0)
        got_f, _ = run(int(d_odd.ptr) + 2, np.float32, offset=31.7, fill=-1.0)
        np.testing.assert_array_equal(got_f.view(np.uint32), want_f.view(np.uint32))
        # bad tables: ValueError before anything is written
        past = srcs.copy()
        past[1]["base"] = len(pool) - 40 * 9 * 4 - 40 * 8 - 32            # its last element is pool[len(pool)]
        zero = srcs.copy()
        zero[2]["ey"] = 0
        high = lists.copy()
        high[2, 1] = len(srcs)
        for kw in ({"lists": high}, {"srcs": past}, {"srcs": zero}, {"fill": 70000}, {"fill": 1.5}):
            with pytest.raises(ValueError):
                run(d_pool, np.uint16, **dict({"fill": 77}, **kw))
            d_out = ctx.alloc(n_out * 2).fill(0xA5)
            try:
                with pytest.raises(ValueError):
                    ctx.gather_boxes(d_pool, len(pool), kw.get("srcs", srcs), kw.get("lists", lists), starts, box, d_out,
                                     np.uint16, fill=kw.get("fill", 77))
                ctx.sync()
                assert np.all(d_out.download((n_out * 2,), np.uint8) == 0xA5)
            finally:
                d_out.free()
        past[1]["base"] -= 1                                               # one element earlier it fits
        np.testing.assert_array_equal(run(d_pool, np.uint16, srcs=past, fill=77)[0],
                                      ref.gather_boxes_ref(pool, past, lists, starts, box, fill=77))
        # no boxes: nothing to do
        ctx.gather_boxes(d_pool, len(pool), srcs, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), box, None)
    finally:
        d_pool.free()
        d_odd.free()


def test_patches_that_stay_on_the_device(stores, ctx):
    path, expected, _ = stores["A-dctq"]
    arr = chunk_store.open_zarr(path)
    host = arr.read_patches(STARTS_A, BOX_A, is_center=False, fill=9)
    dev = arr.read_patches(STARTS_A, BOX_A, is_center=False, fill=9, out="device")
    try:
        assert dev.shape == host.shape and dev.dtype == np.uint16 and dev.data_ptr() == dev.buf.ptr
        np.testing.assert_array_equal(dev.download(), host)
        hist = ctx.u16_histogram(dev, host.size)
        np.testing.assert_array_equal(hist, np.bincount(host.reshape(-1), minlength=65536).astype(np.uint64))
    finally:
        dev.free()
    assert dev.data_ptr() == 0
    none = arr.read_patches(np.zeros((0, 3), int), BOX_A, out="device")
    assert none.shape == (0,) + BOX_A and none.download().shape == (0,) + BOX_A and none.data_ptr() == 0
