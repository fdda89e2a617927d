"""Region reads of a chunk store, the host side (no GPU): the planner against a brute-force enumeration, its tables
through a CPU restatement of the gather kernel, the key normalisation of ``StoredArray.__getitem__`` against numpy,
and the reference's patch-coordinate helpers."""
import numpy as np
import pytest

import region_pyref as ref
from aind_exaspim_image_compression.utils import img_util
from aind_exaspim_image_compression.utils.store_read import normalize_key, plan_read


def _random_case(rng):
    chunk = tuple(int(c) for c in rng.integers(1, 9, 3))
    shape = tuple(int(s) for s in rng.integers(1, 30, 3))
    box = tuple(int(b) for b in rng.integers(1, 40, 3))           # up to larger than the array
    n = int(rng.integers(1, 6))
    starts = np.stack([rng.integers(-box[a] - 3, shape[a] + 4, n) for a in range(3)], axis=1)
    return shape, chunk, box, starts


def _check_groups(groups, shape, chunk, box, starts, nominal):
    """Every property the plan promises, against the brute-force enumeration."""
    assert [g.first for g in groups] == [0] + [g.stop for g in groups[:-1]] and groups[-1].stop == len(starts)
    for g in groups:
        want = sorted({t for n in range(g.first, g.stop) for t in ref.touched_ref(shape, chunk, starts[n], box)})
        assert [tuple(int(v) for v in c) for c in g.chunks] == want
        assert len(g.stacks) <= 8
        seen = sorted(m for st in g.stacks for m in st.members)
        assert seen == list(range(len(g.chunks)))                   # every chunk in exactly one stack
        for st in g.stacks:
            cgrid = tuple(-(-s // c) for s, c in zip(st.shape, st.chunk))
            assert int(np.prod(cgrid)) == len(st.members)
            want_chunk = tuple(chunk) if nominal else tuple(min(c, s) for c, s in zip(chunk, st.shape))
            assert st.chunk == want_chunk
            for k, m in enumerate(st.members):
                # chunk k of the virtual volume, raster order, has the member's true extent ...
                kz, ky, kx = k // (cgrid[1] * cgrid[2]), k // cgrid[2] % cgrid[1], k % cgrid[2]
                ext = tuple(min(c, s - i * c) for i, c, s in zip((kz, ky, kx), st.chunk, st.shape))
                true = tuple(min(c, s - int(i) * c) for i, c, s in zip(g.chunks[m], chunk, shape))
                assert ext == true
                # ... and the source record points at it
                s = g.srcs[m]
                assert (s["ez"], s["ey"], s["ex"]) == true
                assert (s["z0"], s["y0"], s["x0"]) == tuple(int(i) * c for i, c in zip(g.chunks[m], chunk))
                assert (s["stride_z"], s["stride_y"]) == (st.shape[1] * st.shape[2], st.shape[2])
                org = (kz * st.chunk[0], ky * st.chunk[1], kx * st.chunk[2])
                assert s["base"] == st.base + (org[0] * st.shape[1] + org[1]) * st.shape[2] + org[2]
            assert st.base + int(np.prod(st.shape)) <= g.pool_elems
        for n in range(g.first, g.stop):
            mine = [int(k) for k in g.box_srcs[n - g.first] if k >= 0]
            assert [tuple(int(v) for v in g.chunks[k]) for k in mine] == ref.touched_ref(shape, chunk, starts[n], box)


@pytest.mark.parametrize("nominal", [False, True])
def test_planner_against_brute_force(nominal):
    rng = np.random.default_rng(5 + nominal)
    for _ in range(150):
        shape, chunk, box, starts = _random_case(rng)
        groups = plan_read(shape, chunk, starts, box, nominal)
        assert len(groups) == 1
        _check_groups(groups, shape, chunk, box, starts, nominal)
        small = plan_read(shape, chunk, starts, box, nominal, max_pool_bytes=1)
        assert [(g.first, g.stop) for g in small] == [(n, n + 1) for n in range(len(starts))]
        _check_groups(small, shape, chunk, box, starts, nominal)
    # a cap between one box's chunks and all of them: consecutive groups, each under the cap unless a single box
    shape, chunk, box = (40, 40, 40), (8, 8, 8), (8, 8, 8)
    starts = np.array([[0, 0, 0], [0, 0, 4], [8, 8, 8], [8, 8, 12], [30, 30, 30]])
    mid = plan_read(shape, chunk, starts, box, nominal, max_pool_bytes=2 * 2 * 512 + 100)
    assert [(g.first, g.stop) for g in mid] == [(0, 2), (2, 4), (4, 5)]
    _check_groups(mid, shape, chunk, box, starts, nominal)
    assert plan_read(shape, chunk, np.zeros((0, 3), int), box, nominal) == []


def test_all_eight_extent_classes_of_store_a():
    groups = plan_read(ref.SHAPE_A, ref.CHUNK_A, [[-3, -2, -5]], (48, 32, 96), True)
    assert len(groups) == 1 and len(groups[0].chunks) == 18 and len(groups[0].stacks) == 8
    assert groups[0].box_srcs.shape == (1, 18)


@pytest.mark.parametrize("nominal", [False, True])
def test_gather_ref_fed_by_the_planner_equals_padded_slicing(nominal):
    """Pools filled from a numpy array in the place of a decoder: this pins the tables."""
    rng = np.random.default_rng(17)
    for _ in range(60):
        shape, chunk, box, starts = _random_case(rng)
        vol = rng.integers(0, 65536, shape).astype(np.uint16)
        for cap in (1 << 30, 1):
            got = np.empty((len(starts),) + box, dtype=np.uint16)
            for g in plan_read(shape, chunk, starts, box, nominal, max_pool_bytes=cap):
                pool = np.full(g.pool_elems, 0xDEAD, dtype=np.uint16)
                for st in g.stacks:
                    virt = np.empty(st.shape, dtype=np.uint16)
                    for k, m in enumerate(st.members):
                        iz, iy, ix = (int(v) for v in g.chunks[m])
                        c = vol[iz * chunk[0]:(iz + 1) * chunk[0], iy * chunk[1]:(iy + 1) * chunk[1],
                                ix * chunk[2]:(ix + 1) * chunk[2]]
                        at = [0, 0, 0]
                        at[st.axis] = k * chunk[st.axis]
                        virt[at[0]:at[0] + c.shape[0], at[1]:at[1] + c.shape[1], at[2]:at[2] + c.shape[2]] = c
                    pool[st.base:st.base + virt.size] = virt.reshape(-1)
                got[g.first:g.stop] = ref.gather_boxes_ref(pool, g.srcs, g.box_srcs, starts[g.first:g.stop], box,
                                                           fill=7)
            np.testing.assert_array_equal(got, ref.slice_boxes(vol, starts, box, fill=7))


def test_gather_ref_first_source_wins_and_float_offset():
    pool = np.arange(100, dtype=np.uint16)
    srcs = np.zeros(2, dtype=[("base", "<u8"), ("stride_y", "<u8"), ("stride_z", "<u8"), ("z0", "<i4"), ("y0", "<i4"),
                              ("x0", "<i4"), ("ez", "<i4"), ("ey", "<i4"), ("ex", "<i4")])
    srcs[0] = (0, 4, 8, 0, 0, 0, 1, 2, 4)
    srcs[1] = (50, 6, 12, 0, 0, 2, 1, 2, 6)
    out = ref.gather_boxes_ref(pool, srcs, [[0, 1]], [[0, 0, -1]], (1, 2, 10), np.float32, 1.5, -1.0)
    want = np.array([[-1, 0, 1, 2, 3, 52, 53, 54, 55, -1], [-1, 4, 5, 6, 7, 58, 59, 60, 61, -1]], np.float32)
    want[want >= 0] -= np.float32(1.5)
    np.testing.assert_array_equal(out[0, 0], want)
    swapped = ref.gather_boxes_ref(pool, srcs, [[1, 0]], [[0, 0, -1]], (1, 2, 10))
    np.testing.assert_array_equal(swapped[0, 0, 0], [0, 0, 1, 50, 51, 52, 53, 54, 55, 0])


KEYS = [(), 0, (0, 0), (0, 0, 2), (0, 0, -1, 3, -7), (0, 0, slice(1, 4), slice(None), slice(5, None)),
        (0, 0, slice(-3, None), 2, slice(None, -1)), (slice(None), slice(None), slice(2, 100), slice(-100, 2)),
        (0, 0, slice(3, 3)), (0, 0, slice(4, 2)), (slice(1, None),), (0, slice(0, 0)), (0, 0, slice(None, None, 1)),
        (-1, -1, slice(10, 20)), (np.int64(0), 0, np.int32(4)), (0, 0, slice(-2, -1), slice(1, -1), slice(0, 7))]


def test_getitem_key_normalisation_against_numpy():
    a = np.arange(1 * 1 * 5 * 4 * 7).reshape(1, 1, 5, 4, 7)
    for key in KEYS:
        starts, stops, shape = normalize_key(key, a.shape)
        want = a[key]
        assert shape == want.shape, key
        if want.size:
            got = a[tuple(slice(s, e) for s, e in zip(starts, stops))].reshape(shape)
            np.testing.assert_array_equal(got, want)
    for bad in [(0, 0, slice(None, None, 2)), (0, 0, slice(None, None, -1)), (Ellipsis,), (0, 0, None),
                (0, 0, [1, 2]), (0, 0, np.array([1])), (0, 0, 0, 0, 0, 0), (1,), (0, -2), (0, 0, 5), (0, 0, -6),
                (0, 0, 1.0), (True,)]:
        with pytest.raises(IndexError):
            normalize_key(bad, a.shape)


def test_img_util_patch_helpers():
    assert img_util.get_start_end((10, 10, 10), (4, 5, 6)) == ([8, 8, 7], [12, 12, 13])
    # the reference's quirk: the end is voxel + shape // 2 whichever the voxel is
    assert img_util.get_start_end((10, 10, 10), (4, 5, 6), is_center=False) == ((10, 10, 10), [12, 12, 13])
    assert img_util.get_slices((10, 10, 10), (4, 5, 6)) == (slice(8, 12), slice(8, 13), slice(7, 13))
    assert img_util.is_inbounds((0, 4, 6), (1, 5, 7)) and not img_util.is_inbounds((0, 5, 6), (1, 5, 7))
    assert not img_util.is_inbounds((-1, 0, 0), (1, 5, 7))
    img = np.arange(2 * 6 * 8 * 9, dtype=np.uint16).reshape(1, 2, 6, 8, 9)
    np.testing.assert_array_equal(img_util.get_patch(img, (3, 4, 4), (2, 4, 4)), img[0, 0, 2:4, 2:6, 2:6])
    np.testing.assert_array_equal(img_util.get_patch(img, (2, 2, 2), (2, 4, 4), is_center=False),
                                  img[0, 0, 2:3, 2:4, 2:4])
    fallback = img_util.get_patch(img, (-5, -5, -5), (2, 4, 4))
    assert fallback.shape == (2, 4, 4) and fallback.dtype == np.float64 and np.all(fallback == 1)
    assert np.all(img_util.get_patch(img, (20, 20, 20), (2, 4, 4)) == 1)
    with pytest.raises(AssertionError):
        img_util.get_patch(img[0], (3, 4, 4), (2, 4, 4))


def test_open_zarr_reads_the_metadata_only(tmp_path):
    """No chunk file and no device: attributes, the refusals, and the reads that need neither."""
    import json
    import os

    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec

    def store(name, meta):
        os.makedirs(tmp_path / name)
        with open(tmp_path / name / "zarr.json", "w") as f:
            json.dump(meta, f)
        return str(tmp_path / name)

    arr = chunk_store.open_zarr(store("a", chunk_store.metadata((37, 21, 70), (16, 16, 32))))
    assert arr.shape == (1, 1, 37, 21, 70) and arr.chunks == (1, 1, 16, 16, 32) and arr.ndim == 5
    assert arr.dtype == np.uint16 and arr.meta["codecs"][0]["name"] == "exac" and len(arr) == 1
    lossy = chunk_store.open_zarr(store("b", chunk_store.metadata((37, 21, 70), (16, 16, 32),
                                                                   codec=BoundedDctCodec(4))))
    assert lossy.meta["codecs"][0]["name"] == "exac-dctq"
    # empty results and empty batches touch neither a file nor the device
    assert arr[0, 0, 5:5, :, 3:].shape == (0, 21, 67) and arr[0, 0, 40:, 2].shape == (0, 70)
    assert arr[1:].shape == (0, 1, 37, 21, 70)
    empty = arr.read_patches(np.zeros((0, 3), int), (4, 5, 6), dtype=np.float32, offset=2.0)
    assert empty.shape == (0, 4, 5, 6) and empty.dtype == np.float32
    assert arr.last_read["chunks"] == 0 and arr.last_read["groups"] == 0
    for bad in ((0, 0, slice(None, None, 2)), (Ellipsis,), (0, 0, None), (0, 0, [1]), (0, 0, 37)):
        with pytest.raises(IndexError):
            arr[bad]
    with pytest.raises(ValueError):
        arr.read_patches([[0, 0, 0]], (4, 4, 4), offset=1.0)                   # an offset goes with float32
    with pytest.raises(ValueError):
        arr.read_patches([[0, 0, 0]], (4, 4, 4), fill=70000)
    with pytest.raises(ValueError):
        arr.read_patches([[0, 0, 0]], (4, 4, 0))
    with pytest.raises(NotImplementedError):
        chunk_store.open_zarr(store("c", chunk_store.metadata((8, 8, 8), (8, 8, 8), typesize=4)))
    broken = chunk_store.metadata((8, 8, 8), (8, 8, 8))
    broken["codecs"][0]["name"] = "blosc"
    with pytest.raises(ValueError):
        chunk_store.open_zarr(store("d", broken))
    with pytest.raises(FileNotFoundError):
        chunk_store.open_zarr(str(tmp_path / "nowhere"))


def test_read_patches_takes_integer_voxels_only(tmp_path):
    import json
    import os

    from aind_exaspim_image_compression.utils import chunk_store
    os.makedirs(tmp_path / "a")
    with open(tmp_path / "a" / "zarr.json", "w") as f:
        json.dump(chunk_store.metadata((8, 8, 8), (8, 8, 8)), f)
    arr = chunk_store.open_zarr(str(tmp_path / "a"))
    with pytest.raises(ValueError):
        arr.read_patches([[0.5, 1, 2]], (2, 2, 2))
    with pytest.raises(ValueError):
        arr.read_patches([["a", "b", "c"]], (2, 2, 2))
