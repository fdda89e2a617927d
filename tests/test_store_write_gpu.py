"""Region writes of a chunk store on the MI355X: ``Context.scatter_boxes`` against its numpy
restatement, ``StoredArray.write_patches`` / item assignment against numpy assignment and the host coders' bytes, stores
built from nothing against ``write_zarr``, the lossy rule, and ``bm4d.denoise_store`` against ``denoise_chunked`` +
``write_zarr`` and the oracle.  Every comparison is ``array_equal`` or byte equality; every expected value comes from
numpy, the host coders or functions the write side does not touch."""
import os
import shutil

import numpy as np
import pytest

import region_pyref as ref
import region_write_pyref as wref
from util import synth_volume

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.bm4d import denoise_chunked, denoise_store
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
from aind_exaspim_image_compression.utils.store_read import DevicePatches
from test_store_read_gpu import BOX_A, BOX_B, STARTS_A, STARTS_B

pytestmark = pytest.mark.gpu

SIGMA, OFFSET = 24.0, 37.0


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    return ref.build_stores(tmp_path_factory.mktemp("write-stores"))


def _files(path):
    """{relative name: bytes} of every file of a store."""
    out = {}
    for root, _, names in os.walk(path):
        for n in names:
            full = os.path.join(root, n)
            with open(full, "rb") as f:
                out[os.path.relpath(full, path)] = f.read()
    return out


def _stamps(path):
    return {os.path.relpath(os.path.join(r, n), path): (os.stat(os.path.join(r, n)).st_ino,
                                                        os.stat(os.path.join(r, n)).st_mtime_ns)
            for r, _, names in os.walk(path) for n in names}


def _rec(rows):
    t = np.zeros(len(rows), dtype=_native.BOX_SRC)
    for i, r in enumerate(rows):
        t[i] = r
    return t


# ---- the kernel ------------------------------------------------------------------------------------------------
GUARD = 64          # elements on both sides of the pool


def _run_scatter(ctx, src, boxes, pool, dsts, lists, offset=0.0, src_shift=0, pool_shift=0):
    """The entry on device copies of ``src`` and ``pool`` (each ``*_shift`` elements into a larger buffer, guard
    bands around the pool) -> the whole pool afterwards; the guards must be intact."""
    item = pool.dtype.itemsize
    poison = np.frombuffer(bytes([0xA5]) * item, dtype=pool.dtype)[0]
    framed = np.concatenate([np.full(GUARD + pool_shift, poison, pool.dtype), pool, np.full(GUARD, poison, pool.dtype)])
    d_pool = ctx.to_device(framed)
    d_src = ctx.to_device(np.concatenate([np.zeros(src_shift, src.dtype), src.reshape(-1)]))
    try:
        ctx.scatter_boxes(int(d_src.ptr) + src_shift * src.dtype.itemsize, src.size, src.dtype, boxes,
                          int(d_pool.ptr) + (GUARD + pool_shift) * item, pool.size, pool.dtype, dsts, lists, offset)
        ctx.sync()
    finally:
        back = d_pool.download(framed.shape, pool.dtype)
        d_pool.free()
        d_src.free()
    assert np.all(back[:GUARD + pool_shift].view(np.uint8) == 0xA5) and np.all(back[-GUARD:].view(np.uint8) == 0xA5)
    return back[GUARD + pool_shift:-GUARD]


# destinations (base, stride_y, stride_z, z0, y0, x0, ez, ey, ex): two chunks of a stacked virtual volume whose
# strides exceed their extents, a truncated edge chunk at an odd base, a 300-wide one, one no box reaches
DSTS = [(128, 80, 80 * 6, 0, 0, 0, 4, 6, 37), (128 + 37, 80, 80 * 6, 0, 0, 37, 4, 6, 43), (2301, 5, 5 * 3, 4, 0, 0, 2, 3, 5),
        (2400, 300, 300 * 2, 10, 0, 0, 3, 2, 300), (3, 8, 8 * 2, 50, 50, 50, 2, 2, 8)]
POOL_ELEMS = 4400
# boxes (z0, y0, x0, ez, ey, ex): x extents 1, 2, 3, 70 and 300, odd and even x origins, three that overlap one
# another, one that touches no destination
BOX_GEOM = [(0, 0, 0, 3, 4, 70), (1, 1, 5, 2, 2, 3), (1, 2, 6, 4, 3, 2), (2, 2, 7, 1, 1, 1), (0, 3, 36, 6, 3, 3),
            (10, 0, 0, 3, 2, 300), (11, 1, 101, 1, 1, 70), (4, 1, 2, 1, 2, 2), (30, 30, 30, 2, 2, 2), (0, 0, 79, 4, 6, 1)]


def _box_table(shift=0):
    """Records of BOX_GEOM laid out one after another in a source buffer, each row padded by ``shift`` elements."""
    rows, at = [], 0
    for z0, y0, x0, ez, ey, ex in BOX_GEOM:
        sy = ex + shift
        rows.append((at, sy, sy * ey, z0, y0, x0, ez, ey, ex))
        at += sy * ey * ez + shift
    return _rec(rows), at


LISTS = np.array([[0, 1, 2, 3, 4, 9], [0, 4, -1, 9, -1, -1], [7, -1, -1, -1, -1, -1], [-1, 5, -1, 6, -1, -1],
                  [-1, -1, -1, -1, -1, -1]], dtype=np.int32)


@pytest.mark.parametrize("src_shift,pool_shift,row_shift", [(0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)])
def test_scatter_boxes_u16(ctx, src_shift, pool_shift, row_shift):
    rng = np.random.default_rng(3)
    boxes, n_src = _box_table(row_shift)
    src = rng.integers(0, 65536, n_src).astype(np.uint16)
    pool = rng.integers(0, 65536, POOL_ELEMS).astype(np.uint16)
    dsts = _rec(DSTS)
    want = wref.scatter_boxes_ref(src, boxes, pool, dsts, LISTS)
    got = _run_scatter(ctx, src, boxes, pool, dsts, LISTS, src_shift=src_shift, pool_shift=pool_shift)
    np.testing.assert_array_equal(got, want)
    assert np.any(want != pool)
    # the last listed box wins where three overlap; reversing a list changes the result
    rev = LISTS[:, ::-1].copy()
    want_rev = wref.scatter_boxes_ref(src, boxes, pool, dsts, rev)
    assert np.any(want_rev != want)
    np.testing.assert_array_equal(_run_scatter(ctx, src, boxes, pool, dsts, rev, src_shift=src_shift,
                                               pool_shift=pool_shift), want_rev)


def test_scatter_boxes_lists_of_nothing(ctx):
    rng = np.random.default_rng(4)
    boxes, n_src = _box_table()
    src = rng.integers(0, 65536, n_src).astype(np.uint16)
    pool = rng.integers(0, 65536, POOL_ELEMS).astype(np.uint16)
    dsts = _rec(DSTS)
    for lists in (np.zeros((len(DSTS), 0), np.int32), np.full((len(DSTS), 3), -1, np.int32),
                  np.full((len(DSTS), 1), 8, np.int32)):                   # box 8 touches no destination
        np.testing.assert_array_equal(_run_scatter(ctx, src, boxes, pool, dsts, lists), pool)
    np.testing.assert_array_equal(_run_scatter(ctx, src, boxes, pool, dsts[:0], LISTS[:0]), pool)


@pytest.mark.parametrize("offset", [31.7, 0.0])
def test_scatter_boxes_float32_to_counts(ctx, offset):
    special = np.array([-3, -0.5, 0.5, 1.5, 2.5, 65534.5, 65535.5, 7e4, np.inf, -np.inf, np.nan], dtype=np.float32)
    rng = np.random.default_rng(6)
    boxes, n_src = _box_table(1)
    src = rng.uniform(-100, 66000, n_src).astype(np.float32)
    src[::7] = np.resize(special, len(src[::7]))
    src[:len(special)] = special
    pool = rng.integers(0, 65536, POOL_ELEMS).astype(np.uint16)
    dsts = _rec(DSTS)
    want = wref.scatter_boxes_ref(src, boxes, pool, dsts, LISTS, offset)
    for src_shift, pool_shift in ((0, 0), (1, 1), (1, 0)):
        got = _run_scatter(ctx, src, boxes, pool, dsts, LISTS, offset, src_shift=src_shift, pool_shift=pool_shift)
        np.testing.assert_array_equal(got, want)
    # the special values themselves, as one row
    row = _run_scatter(ctx, special, _rec([(0, 11, 11, 0, 0, 0, 1, 1, 11)]), np.zeros(16, np.uint16),
                       _rec([(3, 11, 11, 0, 0, 0, 1, 1, 11)]), np.array([[0]], np.int32), offset)
    np.testing.assert_array_equal(row[3:14], wref.counts_ref(special, offset))
    if offset == 0.0:
        np.testing.assert_array_equal(row[3:14], [0, 0, 0, 2, 2, 65534, 65535, 65535, 65535, 0, 0])


def test_scatter_boxes_bytes(ctx):
    rng = np.random.default_rng(7)
    boxes, n_src = _box_table(1)
    src = rng.integers(0, 256, n_src).astype(np.uint8)
    pool = rng.integers(0, 256, POOL_ELEMS).astype(np.uint8)
    dsts = _rec(DSTS)
    want = wref.scatter_boxes_ref(src, boxes, pool, dsts, LISTS)
    for src_shift, pool_shift in ((0, 0), (1, 0), (0, 1), (3, 3)):
        np.testing.assert_array_equal(_run_scatter(ctx, src, boxes, pool, dsts, LISTS, src_shift=src_shift,
                                                   pool_shift=pool_shift), want)


def test_scatter_boxes_bad_arguments_write_nothing(ctx):
    rng = np.random.default_rng(8)
    boxes, n_src = _box_table()
    src = rng.integers(0, 65536, n_src).astype(np.uint16)
    pool = rng.integers(0, 65536, POOL_ELEMS).astype(np.uint16)
    dsts = _rec(DSTS)
    d_src, d_pool = ctx.to_device(src), ctx.to_device(pool)
    past_box, past_dst, flat, high, low = boxes.copy(), dsts.copy(), dsts.copy(), LISTS.copy(), LISTS.copy()
    past_box[-1]["base"] += 1                                    # the last box's last element is src[n_src]
    past_dst[3]["base"] = POOL_ELEMS - 300 * 2 * 2 - 300 - 299    # its last element is pool[POOL_ELEMS]
    flat[0]["ey"] = 0
    high[2, 1], low[0, 0] = len(boxes), -2
    try:
        def call(b=boxes, d=dsts, lists=LISTS, sdt=np.uint16, pdt=np.uint16, src_ptr=d_src, pool_ptr=d_pool):
            ctx.scatter_boxes(src_ptr, n_src, sdt, b, pool_ptr, POOL_ELEMS, pdt, d, lists)

        for kw in (dict(b=past_box), dict(d=past_dst), dict(d=flat), dict(lists=high), dict(lists=low),
                   dict(sdt=np.uint8), dict(pdt=np.uint8), dict(sdt=np.uint16, pdt=np.float32),
                   dict(src_ptr=int(d_src.ptr) + 1), dict(pool_ptr=int(d_pool.ptr) + 1), dict(lists=LISTS[:4]),
                   dict(src_ptr=None), dict(pool_ptr=None)):
            with pytest.raises(ValueError):
                call(**kw)
            ctx.sync()
            np.testing.assert_array_equal(d_pool.download(pool.shape, np.uint16), pool)
        with pytest.raises(ValueError):
            ctx.scatter_boxes(d_src, n_src, np.float64, boxes, d_pool, POOL_ELEMS, np.uint16, dsts, LISTS)
        past_dst[3]["base"] -= 1                                 # one element earlier it fits
        call(d=past_dst)
        ctx.sync()
        np.testing.assert_array_equal(d_pool.download(pool.shape, np.uint16),
                                      wref.scatter_boxes_ref(src, boxes, pool, past_dst, LISTS))
    finally:
        d_src.free()
        d_pool.free()


# ---- unaligned writes into lossless stores -----------------------------------------------------------------------
def _geometry(name):
    return (ref.SHAPE_A, ref.CHUNK_A, BOX_A, STARTS_A) if name[0] == "A" else (ref.SHAPE_B, ref.CHUNK_B, BOX_B, STARTS_B)


def _check_store(path, model, chunk, kind, touched, before, stamps):
    """The store at ``path`` holds ``model``: ``read_zarr`` says so, every touched file is the host coder's stream of
    the model's chunk and every other file is the one it was (same inode, same mtime)."""
    np.testing.assert_array_equal(chunk_store.read_zarr(path)[0, 0], model)
    blobs = wref.host_blobs(model, chunk, kind)
    after, now = _files(path), _stamps(path)
    assert set(after) == set(before)
    for idx, blob in blobs.items():
        key = chunk_store.chunk_key(*idx)
        if idx in touched:
            assert after[key] == blob, idx
            assert now[key][0] != stamps[key][0], idx               # a new file took its place
        else:
            assert after[key] == before[key] and now[key] == stamps[key], idx
    assert after["zarr.json"] == before["zarr.json"] and now["zarr.json"] == stamps["zarr.json"]
    assert not [n for n in os.listdir(os.path.dirname(os.path.join(path, chunk_store.chunk_key(0, 0, 0))))
                if n.endswith(".tmp")]


@pytest.mark.parametrize("name", ["A-exac2", "A-exac1", "B-exac2"])
def test_unaligned_writes(stores, tmp_path, ctx, name):
    path, expected, _ = stores[name]
    shape, chunk, box, starts = _geometry(name)
    kind = "exac1" if name == "A-exac1" else "exac2"
    rng = np.random.default_rng(17)
    values = rng.integers(0, 65536, (len(starts),) + box).astype(np.uint16)
    values[1] = 200 + rng.integers(0, 9, box)                        # a compressible patch among the noise
    model = wref.assign_boxes(expected, starts, values)
    states = wref.plan_ref(shape, chunk, starts, [box] * len(starts))
    touched = set(states)
    assert 0 < len(touched) < len(stores[name][2]) and "decode" in states.values()

    def fresh(tag):
        copy = str(tmp_path / tag)
        shutil.copytree(path, copy)
        return copy, _files(copy), _stamps(copy)

    # host uint16 patches
    copy, before, stamps = fresh("host")
    arr = chunk_store.open_zarr(copy, mode="r+")
    arr.write_patches(starts, values, is_center=False)
    _check_store(copy, model, chunk, kind, touched, before, stamps)
    lw = arr.last_write
    assert lw["chunks"] == len(touched) and lw["groups"] == 1 and lw["encode_calls"] <= 16
    assert lw["decoded"] == sum(s == "decode" for s in states.values())
    assert lw["chunk_bytes"] == sum(len(_files(copy)[chunk_store.chunk_key(*t)]) for t in touched)
    assert set(lw["seconds"]) == {"files_read", "decode", "scatter", "encode", "files_write"}
    want_files = _files(copy)
    # centred boxes place them as read_patches does: what was written is read back
    centres = [tuple(s + d // 2 for s, d in zip(st, box)) for st in starts]
    np.testing.assert_array_equal(arr.read_patches(centres, box), ref.slice_boxes(model, starts, box))
    # patches that never visit the host
    copy, before, stamps = fresh("device")
    d_values = ctx.to_device(values)
    arr = chunk_store.open_zarr(copy, mode="r+")
    arr.write_patches(centres, DevicePatches(d_values, values.shape, np.uint16))
    d_values.free()
    assert _files(copy) == want_files
    # float32 patches with an offset: stored as rint(clip(v + offset)), computed on the device
    copy, before, stamps = fresh("float")
    as_f32 = values.astype(np.float32) - np.float32(31.7)
    np.testing.assert_array_equal(wref.counts_ref(as_f32, 31.7), values)
    arr = chunk_store.open_zarr(copy, mode="r+")
    arr.write_patches(starts, as_f32, is_center=False, offset=31.7)
    assert _files(copy) == want_files
    # one box a group: chunks are read, changed and written again, the files are the same
    copy, before, stamps = fresh("capped")
    arr = chunk_store.open_zarr(copy, mode="r+", max_pool_bytes=1)
    arr.write_patches(starts, values, is_center=False)
    assert _files(copy) == want_files
    n_inside = sum(bool(ref.touched_ref(shape, chunk, s, box)) for s in starts)
    assert arr.last_write["groups"] == n_inside
    assert arr.last_write["chunks"] == sum(len(ref.touched_ref(shape, chunk, s, box)) for s in starts)


def test_item_assignment_and_failed_writes(stores, tmp_path):
    path, expected, _ = stores["A-exac2"]
    copy = str(tmp_path / "s")
    shutil.copytree(path, copy)
    arr = chunk_store.open_zarr(copy, mode="r+")
    model = expected.copy()
    rng = np.random.default_rng(2)
    block = rng.integers(0, 65536, (1, 1, 27, 21, 5)).astype(np.uint16)
    with pytest.raises(ValueError):
        arr[0, 0, 3:30, :, 65:] = block                             # exactly the result shape
    arr[0, 0, 3:30, :, 65:] = block[0, 0]
    model[3:30, :, 65:] = block[0, 0]
    arr[0, 0, -6:, 2, :-1] = 7                                      # a scalar, an integer index
    model[-6:, 2, :-1] = 7
    arr[0, 0, 5, 6, 33] = 65535
    model[5, 6, 33] = 65535
    arr[0, 0, 0:2, 0:3, 0:4] = np.float32(2.5)                      # floats are rounded to even
    model[0:2, 0:3, 0:4] = 2
    np.testing.assert_array_equal(chunk_store.read_zarr(copy)[0, 0], model)
    blobs = wref.host_blobs(model, ref.CHUNK_A)
    files = _files(copy)
    assert all(files[chunk_store.chunk_key(*idx)] == b for idx, b in blobs.items())
    # a touched chunk that cannot be decoded: the write raises, nothing is replaced, last_write is None
    victim = os.path.join(copy, chunk_store.chunk_key(0, 0, 1))
    with open(victim, "wb") as f:
        f.write(b"\xff" + files[chunk_store.chunk_key(0, 0, 1)][1:])
    before = _files(copy)
    with pytest.raises(ValueError):
        arr[0, 0, 1:9, 1:9, 20:40] = 1
    assert arr.last_write is None and _files(copy) == before


# ---- a store built from nothing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exac", "dctq", "block"])
def test_a_store_built_by_aligned_slabs_equals_write_zarr(tmp_path, kind):
    vol = ref.volume(ref.SHAPE_A, 32)
    mask = np.zeros(ref.SHAPE_A, dtype=bool)
    mask[ref.MASK_A] = True
    codec = {"exac": ExacCodec(2), "dctq": BoundedDctCodec(4), "block": BlockBoundedCodec(6, 0)}[kind]
    chunks = (1, 1) + ref.CHUNK_A
    whole, built = str(tmp_path / "whole"), str(tmp_path / "built")
    chunk_store.write_zarr(vol, whole, chunks, codec=codec, attributes={"a": 1},
                           **({"mask": mask} if kind == "block" else {}))
    arr = chunk_store.create_zarr(built, ref.SHAPE_A, chunks, codec=codec, attributes={"a": 1})
    # slabs of one chunk layer along z, cut at x = 32 as well: aligned to the grid or the array's edge
    n = 0
    for z0 in range(0, ref.SHAPE_A[0], 16):
        for x0, x1 in ((0, 32), (32, ref.SHAPE_A[2])):
            z1 = min(z0 + 16, ref.SHAPE_A[0])
            if kind == "block":
                arr.write_patches([(z0, 0, x0)], vol[None, z0:z1, :, x0:x1], is_center=False,
                                  mask=mask[None, z0:z1, :, x0:x1])
            else:
                arr[0, 0, z0:z1, :, x0:x1] = vol[z0:z1, :, x0:x1]
            assert arr.last_write["decoded"] == 0
            n += arr.last_write["chunks"]
    assert n == 18
    assert _files(built) == _files(whole)


def test_an_unaligned_write_into_an_empty_store_leaves_zeros(tmp_path):
    path = str(tmp_path / "s")
    arr = chunk_store.create_zarr(path, ref.SHAPE_A, (1, 1) + ref.CHUNK_A)
    rng = np.random.default_rng(9)
    block = rng.integers(1, 65536, (7, 6, 9)).astype(np.uint16)
    arr[0, 0, 12:19, 13:19, 28:37] = block
    model = np.zeros(ref.SHAPE_A, np.uint16)
    model[12:19, 13:19, 28:37] = block
    touched = ref.touched_ref(ref.SHAPE_A, ref.CHUNK_A, (12, 13, 28), block.shape)
    assert len(touched) == 8 and arr.last_write["chunks"] == 8 and arr.last_write["decoded"] == 0
    blobs = wref.host_blobs(model, ref.CHUNK_A)
    files = _files(path)
    assert set(files) == {"zarr.json"} | {chunk_store.chunk_key(*t) for t in touched}
    assert all(files[chunk_store.chunk_key(*t)] == blobs[t] for t in touched)
    got = chunk_store.open_zarr(path).read_patches([(12, 0, 16)], (20, 21, 32), is_center=False)[0]
    np.testing.assert_array_equal(got, model[12:32, :, 16:48])
    with pytest.raises(FileNotFoundError):                           # reading a chunk that was never written
        chunk_store.open_zarr(path)[0, 0, 33:36, 0:4, 0:4]


# ---- the lossy rule -------------------------------------------------------------------------------------------------
def test_a_lossy_store_takes_whole_chunks_only(stores, tmp_path):
    path, expected, _ = stores["A-dctq"]
    copy = str(tmp_path / "s")
    shutil.copytree(path, copy)
    before, stamps = _files(copy), _stamps(copy)
    arr = chunk_store.open_zarr(copy, mode="r+")
    with pytest.raises(ValueError, match="chunk"):
        arr[0, 0, 0:16, 0:16, 0:31] = 5
    with pytest.raises(ValueError, match="chunk"):
        arr.write_patches(STARTS_A, np.zeros((len(STARTS_A),) + BOX_A, np.uint16), is_center=False)
    assert arr.last_write is None and _files(copy) == before and _stamps(copy) == stamps
    # aligned to the grid and to the array's edge: the streams are the Python reference's
    vol = ref.volume(ref.SHAPE_A, 32, seed=12)
    arr[0, 0, 16:37, 0:16, 32:70] = vol[16:37, 0:16, 32:70]
    touched = {(z, 0, x) for z in (1, 2) for x in (1, 2)}
    assert arr.last_write["chunks"] == 4 and arr.last_write["decoded"] == 0
    after = _files(copy)
    want = wref.host_blobs(vol, ref.CHUNK_A, "dctq")                 # a chunk's stream depends on the chunk alone
    for key in after:
        idx = tuple(int(p) for p in key.split(os.sep)[3:]) if key != "zarr.json" else None
        assert after[key] == (want[idx] if idx in touched else before[key]), key


# ---- denoise_store --------------------------------------------------------------------------------------------------
SHAPE_D = (40, 24, 36)


@pytest.fixture(scope="module")
def denoise_case(tmp_path_factory, oracle):
    """The source store, its volume, ``denoise_chunked`` of it (computed once) and the oracle's result."""
    vol, _ = synth_volume(SHAPE_D, as_u16=True)
    src = str(tmp_path_factory.mktemp("denoise") / "src")
    chunk_store.write_zarr(vol, src, (1, 1, 16, 16, 32))
    want = denoise_chunked(vol, SIGMA, OFFSET, chunk=16, halo=4)
    np.testing.assert_array_equal(want, oracle.bm4d_u16_chunked(vol, SIGMA, OFFSET, 16, 4))
    want.setflags(write=False)
    return src, vol, want


def test_denoise_store(denoise_case, tmp_path):
    src, vol, want = denoise_case
    before, stamps = _files(src), _stamps(src)
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    stats = {}
    ratio = denoise_store(src, one, SIGMA, OFFSET, chunk=16, halo=4, chunks=(1, 1, 8, 8, 16), attributes={"k": "v"},
                          stats=stats)
    assert stats["windows"] == 18 and stats["bricks"] == 1 and stats["largest_alloc"] > 0
    assert set(stats["seconds"]) == {"read", "denoise", "scatter", "encode", "files_write"}
    np.testing.assert_array_equal(chunk_store.read_zarr(one)[0, 0], want)
    # chunk file for chunk file what write_zarr makes of denoise_chunked's result, and what the host coder makes
    whole = str(tmp_path / "whole")
    want_ratio = chunk_store.write_zarr(want, whole, (1, 1, 8, 8, 16), attributes={"k": "v"})
    files = _files(one)
    assert files == _files(whole) and ratio == want_ratio
    blobs = wref.host_blobs(np.asarray(want), (8, 8, 16))
    assert len(blobs) == 5 * 3 * 3 == len(files) - 1
    assert all(files[chunk_store.chunk_key(*idx)] == b for idx, b in blobs.items())
    # a budget of one core a brick: the same files
    stats = {}
    denoise_store(chunk_store.open_zarr(src), many, SIGMA, OFFSET, chunk=16, halo=4, chunks=(1, 1, 8, 8, 16),
                  attributes={"k": "v"}, budget_bytes=1 << 20, stats=stats)
    assert stats["bricks"] >= 3 and stats["windows"] == 18
    assert _files(many) == files
    assert _files(src) == before and _stamps(src) == stamps


def test_denoise_store_bounded_codec(denoise_case, tmp_path):
    src, vol, want = denoise_case
    dst = str(tmp_path / "dst")
    denoise_store(src, dst, SIGMA, OFFSET, chunk=16, halo=4, chunks=(1, 1, 8, 8, 16), codec=BoundedDctCodec(4),
                  budget_bytes=24 << 20)
    blobs = wref.host_blobs(np.asarray(want), (8, 8, 16), "dctq")
    files = _files(dst)
    assert len(files) == len(blobs) + 1
    assert all(files[chunk_store.chunk_key(*idx)] == b for idx, b in blobs.items())


def test_denoise_store_under_poisson_gaussian_noise(denoise_case, tmp_path):
    src, vol, _ = denoise_case
    noise = {"gain": 2.0, "read_noise": 3.0, "offset": 37.0}
    dst = str(tmp_path / "dst")
    denoise_store(src, dst, noise=noise, chunk=16, halo=4, chunks=(1, 1, 8, 8, 16), budget_bytes=24 << 20)
    want = denoise_chunked(vol, noise=noise, chunk=16, halo=4)
    np.testing.assert_array_equal(chunk_store.read_zarr(dst)[0, 0], want)
    blobs = wref.host_blobs(want, (8, 8, 16))
    files = _files(dst)
    assert all(files[chunk_store.chunk_key(*idx)] == b for idx, b in blobs.items())
