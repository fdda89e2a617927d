"""Pyramid levels of a store on the MI355X: ``exabm4d_downsample_box_u16_dev`` in guarded, poisoned
buffers against the numpy rule (``pyramid_pyref``) -- every method, edge and factor, windows of every alignment, windows
that reach past the volume's faces (padded with 65535, which a ``"max"`` or ``"mode"`` that read it would show at once),
odd boxes --, the argument checks, a partition with odd corners, ``downsample_volume``, ``downsample_store`` against
``write_zarr`` chunk file for chunk file, and ``pyramid_store`` level by level with its group document."""
import itertools
import json
import os

import numpy as np
import pytest

import measure_pyref
import pyramid_pyref as ref
from util import GuardedView

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import chunk_store, store_pyramid
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec

pytestmark = pytest.mark.gpu
U16 = np.uint16
SHAPE_A, SHAPE_B, SHAPE_C = (22, 19, 27), (9, 10, 131), (16, 16, 64)
FACTORS = [(2, 2, 2), (1, 2, 2), (2, 2, 1), (2, 1, 1)]
MASK_VALUE = 40000
_CACHE = {}


def _window(vol, origin, dims):
    """The window ``origin + [0, dims)`` of ``vol``; what lies past the volume's faces holds 65535."""
    out = np.full(dims, 65535, dtype=U16)
    inside = tuple(slice(0, min(d, n - o)) for o, d, n in zip(origin, dims, vol.shape))
    out[inside] = vol[tuple(slice(o, o + s.stop) for o, s in zip(origin, inside))]
    return out


def _volumes(shape):
    """Named volumes of ``shape``, read-only and made once."""
    if shape not in _CACHE:
        rng = np.random.default_rng(sum(shape))
        n = int(np.prod(shape))
        assert n < 65536
        vols = {"values 0..3 (ties everywhere)": rng.integers(0, 4, shape).astype(U16),
                "ramp (all distinct)": np.arange(n, dtype=U16).reshape(shape),
                "noise": rng.integers(0, 65536, shape).astype(U16),
                "mask at density 0.01": (rng.random(shape) < 0.01).astype(U16) * MASK_VALUE}
        for v in vols.values():
            v.setflags(write=False)
        _CACHE[shape] = vols
    return _CACHE[shape]


def _levels(shape, name, factors, method, edge):
    """The pyref level of a named volume, computed once and shared."""
    key = (shape, name, factors, method, edge)
    if key not in _CACHE:
        level = ref.downsample(_volumes(shape)[name], factors, method, edge)
        level.setflags(write=False)
        _CACHE[key] = level
    return _CACHE[key]


def _box_of(shape, w0, wd, factors, edge):
    """The largest box of the level whose source voxels, cut at the volume, the window holds; None without one."""
    level = ref.level_shape(shape, factors, edge)
    b0 = tuple(-(-o // f) for o, f in zip(w0, factors))
    b1 = tuple(l if o + d >= n else min(l, (o + d) // f) for o, d, n, f, l in zip(w0, wd, shape, factors, level))
    if any(h <= l for l, h in zip(b0, b1)):
        return None
    return b0, tuple(h - l for l, h in zip(b0, b1))


def _run(ctx, shape, name, w0, wd, b0, bd, factors, method, edge, k=0, out_k=0, what=""):
    """One call in guarded, poisoned buffers, checked against the pyref."""
    vol = _volumes(shape)[name]
    want = ref.box(_levels(shape, name, factors, method, edge), b0, bd)
    assert want.shape == tuple(bd)
    win = GuardedView(ctx, U16, int(np.prod(wd)), k=k, data=_window(vol, w0, wd))
    out = GuardedView(ctx, U16, int(np.prod(bd)), k=out_k)
    try:
        ctx.downsample_box_u16(win.ptr, shape, w0, wd, b0, bd, factors, method, edge, out.ptr)
        ctx.sync()
        out.check_output(want, f"{what}: out_u16")
        win.check_untouched(f"{what}: window")
    finally:
        win.free()
        out.free()
    return want


# ---- the entry against the pyref: the largest box of a window -------------------------------------------------------------
# (shape, window origin, window dims -- SOURCE coordinates --, element offset of the window's pointer, of the output's)
SINGLE = {
    "A whole, pitch 27 (element loads)": (SHAPE_A, (0, 0, 0), (22, 19, 27), 0, 0),
    "A past the x face, pitch 32 (vector loads)": (SHAPE_A, (0, 0, 0), (22, 19, 32), 0, 0),
    "A past the x face, pointers + 1 element": (SHAPE_A, (0, 0, 0), (22, 19, 32), 1, 1),
    "A past the x face, window + 2 elements, output + 1": (SHAPE_A, (0, 0, 0), (22, 19, 32), 2, 1),
    "A past the +x +y +z faces, pitch 32": (SHAPE_A, (0, 0, 0), (24, 20, 32), 0, 0),
    "A window at odd (1, 1, 3) to the faces, pitch 24 (first source x odd in the window)": (SHAPE_A, (1, 1, 3), (21, 18, 24), 0, 0),
    "A window at odd (1, 1, 3) past the +x +y +z faces, pitch 32, output + 3": (SHAPE_A, (1, 1, 3), (24, 20, 32), 0, 3),
    "A window at odd (1, 1, 3), pitch 32, pointer + 1 (first source x even in memory)": (SHAPE_A, (1, 1, 3), (24, 20, 32), 1, 0),
    "A inner window (2, 1, 3), pitch 22 (element loads)": (SHAPE_A, (2, 1, 3), (18, 17, 22), 0, 0),
    "A inner window (2, 2, 2), pitch 24, pointer + 1": (SHAPE_A, (2, 2, 2), (18, 16, 24), 1, 0),
    "B whole, pitch 131 (element loads)": (SHAPE_B, (0, 0, 0), (9, 10, 131), 0, 0),
    "B past the faces, pitch 136 (vector loads)": (SHAPE_B, (0, 0, 0), (10, 12, 136), 0, 0),
    "B past the faces, pitch 136, pointers + 1 element": (SHAPE_B, (0, 0, 0), (10, 12, 136), 1, 1),
    "C whole, pitch 64 (vector loads and stores)": (SHAPE_C, (0, 0, 0), (16, 16, 64), 0, 0),
    "C inner window (4, 2, 8), pitch 48, output + 4": (SHAPE_C, (4, 2, 8), (10, 12, 48), 0, 4),
}


@pytest.mark.parametrize("factors", FACTORS, ids=str)
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_box(ctx, case, factors):
    shape, w0, wd, k, out_k = SINGLE[case]
    past = any(o + d > n for o, d, n in zip(w0, wd, shape))
    for edge in ref.EDGES:
        b0, bd = _box_of(shape, w0, wd, factors, edge)
        for method in ref.METHODS:
            for name in _volumes(shape):
                want = _run(ctx, shape, name, w0, wd, b0, bd, factors, method, edge, k=k, out_k=out_k,
                            what=f"{case}, {name}, {factors} {method} {edge}")
                if past and name == "mask at density 0.01" and method != "mean":
                    # a kernel that let the 65535 past the faces in would show it under "max": the pyref holds none
                    assert int(want.max()) in (0, MASK_VALUE)


# boxes whose x extent is no multiple of 4 (nor of 8), at odd corners, down to one voxel -- LEVEL coordinates
ODD_BOXES = [((0, 0, 0), (1, 1, 1)), ((3, 2, 5), (1, 1, 1)), ((1, 0, 2), (5, 9, 7)), ((0, 0, 1), (2, 3, 6)),
             ((4, 3, 0), (3, 2, 13)), ((2, 1, 3), (4, 4, 9)), ((0, 5, 7), (9, 2, 5)), ((8, 8, 12), (1, 1, 1))]


@pytest.mark.parametrize("out_k", (0, 1, 2))
@pytest.mark.parametrize("factors", FACTORS, ids=str)
def test_odd_boxes(ctx, factors, out_k):
    for wd in ((22, 19, 27), (22, 19, 32)):
        for b0, bd in ODD_BOXES:
            for method, edge in (("mode", "crop"), ("mean", "partial"), ("max", "partial")):
                level = ref.level_shape(SHAPE_A, factors, edge)
                assert all(o + d <= l for o, d, l in zip(b0, bd, level))
                for name in ("values 0..3 (ties everywhere)", "noise"):
                    _run(ctx, SHAPE_A, name, (0, 0, 0), wd, b0, bd, factors, method, edge, out_k=out_k,
                         what=f"box {b0} + {bd}, pitch {wd[2]}, {factors} {method} {edge}, output + {out_k}")


def test_the_last_voxels_of_a_partial_level(ctx):
    """One-voxel boxes at the far corner: windows of 1, 2 and 4 voxels beside a reader's padding."""
    for shape, wd in ((SHAPE_A, (24, 20, 32)), (SHAPE_B, (10, 12, 136))):
        for factors in FACTORS + [(1, 1, 2), (1, 2, 1)]:
            level = ref.level_shape(shape, factors, "partial")
            b0 = tuple(l - 1 for l in level)
            for method in ref.METHODS:
                for name in _volumes(shape):
                    _run(ctx, shape, name, (0, 0, 0), wd, b0, (1, 1, 1), factors, method, "partial",
                         what=f"{shape} last voxel, {name}, {factors} {method}")


@pytest.mark.parametrize("method", ref.METHODS)
def test_more_than_one_block_along_every_axis(ctx, method):
    """Rows of more than 64 pieces (x), more rows than a block holds (y) and several layers (z)."""
    shape = (5, 7, 1100)
    rng = np.random.default_rng(9)
    vol = rng.integers(0, 5, shape).astype(U16)
    for factors, edge in (((2, 2, 2), "partial"), ((2, 2, 1), "crop"), ((1, 1, 2), "crop")):
        level = ref.level_shape(shape, factors, edge)
        want = ref.downsample(vol, factors, method, edge)
        win = GuardedView(ctx, U16, vol.size, data=vol)
        out = GuardedView(ctx, U16, want.size)
        try:
            ctx.downsample_box_u16(win.ptr, shape, (0, 0, 0), shape, (0, 0, 0), level, factors, method, edge, out.ptr)
            ctx.sync()
            out.check_output(want, f"{shape} {factors} {method} {edge}")
            win.check_untouched("window")
        finally:
            win.free()
            out.free()


# ---- a partition with odd corners ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factors, edge", [((2, 2, 2), "partial"), ((2, 2, 2), "crop"), ((1, 2, 2), "partial"), ((2, 2, 1), "crop")],
                         ids=str)
def test_partition(ctx, factors, edge):
    name = "values 0..3 (ties everywhere)"
    level = ref.level_shape(SHAPE_A, factors, edge)
    cuts = ([3, 8] if level[0] > 8 else [3], [5], [2, 7, 9])
    for method in ref.METHODS:
        whole = _levels(SHAPE_A, name, factors, method, edge)
        got = np.zeros(level, dtype=U16)
        for i, (b0, bd) in enumerate(measure_pyref.partition(level, cuts)):
            w0 = tuple(o * f for o, f in zip(b0, factors))
            w1 = tuple(min(n, (o + d) * f) for o, d, f, n in zip(b0, bd, factors, SHAPE_A))
            part = _run(ctx, SHAPE_A, name, w0, tuple(h - l for l, h in zip(w0, w1)), b0, bd, factors, method, edge,
                        what=f"box {i}")
            got[tuple(slice(o, o + d) for o, d in zip(b0, bd))] = part
        np.testing.assert_array_equal(got, whole)


# ---- geometry and argument errors -----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    shape, factors = SHAPE_A, (2, 2, 2)
    b0, bd = (2, 2, 2), (5, 4, 6)                          # source voxels (4, 4, 4) + (10, 8, 12)
    w0, wd = (3, 3, 3), (12, 10, 14)
    win = GuardedView(ctx, U16, int(np.prod(wd)) + 8, data=np.zeros(int(np.prod(wd)) + 8, dtype=U16))
    out = GuardedView(ctx, U16, int(np.prod(bd)) + 1)

    def call(shape=shape, w0=w0, wd=wd, b0=b0, bd=bd, factors=factors, method="mode", edge="crop", pw=win.ptr, po=out.ptr):
        ctx.downsample_box_u16(pw, shape, w0, wd, b0, bd, factors, method, edge, po)

    def changed(t, a, by):
        t = list(t)
        t[a] += by
        return tuple(t)

    try:
        call()                                            # the geometry itself is accepted
        ctx.sync()
        out.buf.upload(out.host)                          # poison it again
        bad = [dict(pw=None), dict(po=None), dict(pw=win.ptr + 1), dict(po=out.ptr + 1),
               dict(factors=(1, 1, 1)), dict(factors=(2, 3, 2)), dict(factors=(0, 2, 2)), dict(factors=(2, 2, 4)),
               dict(method="median"), dict(method=3), dict(method=-1), dict(edge="pad"), dict(edge=2), dict(edge=-1),
               dict(shape=((1 << 20) + 1, 19, 27)), dict(shape=(1 << 20, 1 << 20, 2))]
        for a in range(3):
            bad += [dict(w0=changed(w0, a, 2), wd=changed(wd, a, -2)),        # the window begins after the box's source
                    dict(wd=changed(wd, a, -(wd[a] - (bd[a] * 2 + 1)) - 1)),   # the window ends one voxel too early
                    dict(bd=changed(bd, a, -bd[a])), dict(wd=changed(wd, a, -wd[a])), dict(shape=changed(shape, a, -shape[a])),
                    dict(b0=changed(b0, a, -3)),                               # a negative origin
                    dict(w0=changed(w0, a, -4)),                               # the window begins before the volume
                    dict(b0=changed(b0, a, shape[a] // 2 - b0[a] - bd[a] + 1), w0=(0, 0, 0), wd=shape)]   # past the crop level
        # the last voxel of the "partial" level does not exist under "crop" (22 x 19 x 27: z is even, y and x are odd)
        bad += [dict(b0=(0, 9, 0), bd=(1, 1, 1), w0=(0, 0, 0), wd=shape), dict(b0=(0, 0, 13), bd=(1, 1, 1), w0=(0, 0, 0), wd=shape)]
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        # a NULL geometry pointer, past the wrapper
        tri = ctx._box_geometry(shape, w0, wd, b0, bd)
        fac = (_native.ctypes.c_int32 * 3)(2, 2, 2)
        fn = _native.lib().exabm4d_downsample_box_u16_dev
        for i in range(6):
            args = list(tri) + [fac]
            args[i] = None
            assert fn(ctx.handle, win.ptr, *args, 0, 0, out.ptr) == -1
        ctx.sync()
        out.check_untouched("after the refused calls")
        win.check_untouched("after the refused calls")
        call(b0=(0, 9, 13), bd=(1, 1, 1), w0=(0, 18, 26), wd=(2, 1, 1), edge="partial")         # accepted under "partial"
        ctx.sync()
    finally:
        win.free()
        out.free()


# ---- downsample_volume ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (SHAPE_A, SHAPE_B, SHAPE_C), ids=str)
def test_downsample_volume_is_the_pyref(shape):
    for name, vol in _volumes(shape).items():
        for factors, method, edge in itertools.product(((2, 2, 2), (1, 2, 2)), ref.METHODS, ref.EDGES):
            got = store_pyramid.downsample_volume(vol, factors, method, edge)
            assert got.dtype == U16
            np.testing.assert_array_equal(got, _levels(shape, name, factors, method, edge),
                                          err_msg=f"{name} {factors} {method} {edge}")


# ---- downsample_store against write_zarr, chunk file for chunk file -----------------------------------------------------------
STORE_SHAPE, SRC_CHUNKS, DST_CHUNKS = (45, 38, 67), (1, 1, 16, 16, 32), (1, 1, 8, 8, 16)
BUDGETS = {"one brick": 4 << 30, "one chunk per brick": 1}


def _files(path):
    out = {}
    for dirpath, _, names in os.walk(path):
        for name in names:
            full = os.path.join(dirpath, name)
            with open(full, "rb") as f:
                out[os.path.relpath(full, path)] = f.read()
    return out


def _assert_same_store(got, want, what):
    a, b = _files(got), _files(want)
    assert sorted(a) == sorted(b), f"{what}: the directory listings differ"
    assert len(a) > 1 and "zarr.json" in a
    for name in a:
        assert a[name] == b[name], f"{what}: {name} differs"


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """The source store and what ``read_zarr`` gives back of it, made once."""
    root = tmp_path_factory.mktemp("pyramid_store")
    rng = np.random.default_rng(21)
    vol = rng.poisson(6, STORE_SHAPE).astype(U16)          # few values: ties in most windows
    vol[10:14, 8:30, 20:50] += rng.integers(300, 3000, (4, 22, 30)).astype(U16)
    vol[-1, -1, -1] = vol[0, -1, -1] = 65535
    vol.setflags(write=False)
    src = str(root / "src")
    chunk_store.write_zarr(vol, src, SRC_CHUNKS)
    back = chunk_store.read_zarr(src)[0, 0]
    np.testing.assert_array_equal(back, vol)
    return {"root": root, "vol": back, "src": src}


@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("method", ref.METHODS)
def test_downsample_store_is_write_zarr_of_the_level(stored, method, edge, tmp_path):
    level = ref.downsample(stored["vol"], (2, 2, 2), method, edge)
    want = str(tmp_path / "want")
    ratio = chunk_store.write_zarr(level, want, DST_CHUNKS)
    bricks = {}
    for budget in BUDGETS:
        st = {}
        dst = str(tmp_path / f"dst_{len(bricks)}")
        res = chunk_store.downsample_store(stored["src"], dst, (2, 2, 2), method, edge, chunks=DST_CHUNKS,
                                           budget_bytes=BUDGETS[budget], stats=st)
        _assert_same_store(dst, want, f"{method} {edge}, {budget}")
        assert res == {"shape": level.shape, "n": level.size, "cratio": ratio}
        assert set(st["seconds"]) == {"read", "reduce", "scatter", "encode", "files_write"}
        assert st["voxels_read"] == int(np.prod([min(n, l * 2) for n, l in zip(STORE_SHAPE, level.shape)]))
        assert st["largest_alloc"] > 0
        bricks[budget] = st["bricks"]
    grid = [-(-s // c) for s, c in zip(level.shape, DST_CHUNKS[2:])]
    assert bricks["one brick"] == 1 < bricks["one chunk per brick"] == int(np.prod(grid))


def test_downsample_store_with_other_factors_a_lossy_codec_and_a_mask(stored, tmp_path):
    # per-axis factors, several chunks per brick
    level = ref.downsample(stored["vol"], (1, 2, 2), "mode", "partial")
    want, dst = str(tmp_path / "want_122"), str(tmp_path / "dst_122")
    chunk_store.write_zarr(level, want, DST_CHUNKS)
    st = {}
    chunk_store.downsample_store(stored["src"], dst, (1, 2, 2), "mode", "partial", chunks=DST_CHUNKS, budget_bytes=60_000,
                                 stats=st)
    _assert_same_store(dst, want, "(1, 2, 2) mode partial")
    assert 1 < st["bricks"] < int(np.prod([-(-s // c) for s, c in zip(level.shape, DST_CHUNKS[2:])]))
    # the bounded lossy codec as the destination's
    level = ref.downsample(stored["vol"], (2, 2, 2), "mean", "crop")
    want, dst = str(tmp_path / "want_dct"), str(tmp_path / "dst_dct")
    chunk_store.write_zarr(level, want, DST_CHUNKS, codec=BoundedDctCodec(3))
    chunk_store.downsample_store(stored["src"], dst, (2, 2, 2), "mean", "crop", chunks=DST_CHUNKS, codec=BoundedDctCodec(3),
                                 budget_bytes=1)
    _assert_same_store(dst, want, "mean crop, BoundedDctCodec(3)")
    # a foreground_store mask under "max": any voxel set, and the mask's value survives
    mask = str(tmp_path / "mask")
    res = metrics.foreground_store(stored["src"], mask, k=4, dilate=1, value=MASK_VALUE)
    assert 0 < res["n_fg"] < res["n"]
    level = ref.downsample(chunk_store.read_zarr(mask)[0, 0], (2, 2, 2), "max", "partial")
    assert set(np.unique(level)) == {0, MASK_VALUE}
    want, dst = str(tmp_path / "want_mask"), str(tmp_path / "dst_mask")
    chunk_store.write_zarr(level, want, DST_CHUNKS)
    chunk_store.downsample_store(mask, dst, (2, 2, 2), "max", "partial", chunks=DST_CHUNKS, budget_bytes=1)
    _assert_same_store(dst, want, "a mask under max")


# ---- pyramid_store ----------------------------------------------------------------------------------------------------------------
def test_pyramid_store_level_by_level(stored, tmp_path):
    dst, want0 = str(tmp_path / "pyramid"), str(tmp_path / "want0")
    steps = [(1, 2, 2), (2, 2, 2)]
    st = {}
    res = chunk_store.pyramid_store(stored["src"], dst, 3, steps, "mode", "partial", chunks=DST_CHUNKS,
                                    voxel_size=(3, 4, 5), budget_bytes=60_000, stats=st)
    chunk_store.recode_store(stored["src"], want0, chunks=DST_CHUNKS)
    _assert_same_store(os.path.join(dst, "0"), want0, "level 0")
    levels, transforms = chunk_store.open_multiscale(dst)
    assert len(levels) == 3 and len(st["levels"]) == 3
    before = stored["vol"]
    for k, arr in enumerate(levels):
        got = chunk_store.read_zarr(os.path.join(dst, str(k)))[0, 0]
        if k:
            before = ref.downsample(before, steps[k - 1], "mode", "partial")
        np.testing.assert_array_equal(got, before, err_msg=f"level {k}")
        assert tuple(arr.shape) == (1, 1) + before.shape == (1, 1) + res["shapes"][k]
    assert res["shapes"] == [(45, 38, 67), (45, 19, 34), (23, 10, 17)]
    assert transforms == res["transforms"] == store_pyramid.level_transforms(steps, voxel_size=(3, 4, 5))
    assert transforms[2] == ([1.0, 1.0, 10.0, 16.0, 12.0], [0.0, 0.0, 2.5, 6.0, 4.5])
    with open(os.path.join(dst, "zarr.json")) as f:
        doc = json.load(f)
    assert doc == store_pyramid.group_document(transforms, "mode")
    assert doc["attributes"]["ome"]["multiscales"][0]["type"] == "mode"
    # one triple, "crop": 45 x 38 x 67 -> 22 x 19 x 33 -> 11 x 9 x 16
    dst2 = str(tmp_path / "pyramid_crop")
    res = chunk_store.pyramid_store(stored["src"], dst2, 3, chunks=DST_CHUNKS)
    assert res["shapes"] == [(45, 38, 67), (22, 19, 33), (11, 9, 16)]
    level2 = ref.downsample(ref.downsample(stored["vol"], (2, 2, 2)), (2, 2, 2))
    np.testing.assert_array_equal(chunk_store.read_zarr(os.path.join(dst2, "2"))[0, 0], level2)
    # a level count that would empty an axis raises and leaves no directory behind
    with pytest.raises(ValueError):
        chunk_store.pyramid_store(stored["src"], str(tmp_path / "too_deep"), 7, chunks=DST_CHUNKS)
    assert not (tmp_path / "too_deep").exists()
