"""The foreground mask of a store on the MI355X: ``exabm4d_foreground_box_u16_dev`` in guarded,
poisoned buffers against the numpy restatement (``foreground_pyref.box_mask``, the L1-ball definition) -- windows of
every alignment, windows that reach past the volume's faces, every radius, seeds where the packed words and the regions
meet --, a partition with odd corners, the argument checks, ``foreground_volume`` against the per-patch kernels,
``foreground_store`` and ``recode_store`` against ``write_zarr`` file for file, and the uint16 -> byte mask conversion."""
import os

import numpy as np
import pytest

import foreground_pyref as ref
import mask_pyref
import measure_pyref
from util import GuardedView

from aind_exaspim_image_compression import _native, evaluate
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import chunk_store, noise, store_foreground
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec

pytestmark = pytest.mark.gpu
U16 = np.uint16
RADII = (0, 1, 2, 3, 8)
SHAPE_A, SHAPE_B = (22, 19, 27), (9, 10, 131)
_CACHE = {}


def _window(vol, origin, dims):
    """The window ``origin + [0, dims)`` of ``vol``; what lies past the volume's faces holds 65535."""
    out = np.full(dims, 65535, dtype=U16)
    inside = tuple(slice(0, min(d, n - o)) for o, d, n in zip(origin, dims, vol.shape))
    out[inside] = vol[tuple(slice(o, o + s.stop) for o, s in zip(origin, inside))]
    return out


def _box_of(shape, w0, wd, r):
    """The largest box whose ball of radius ``r``, cut at the volume, the window holds."""
    b0 = tuple(0 if o == 0 else o + r for o in w0)
    b1 = tuple(n if o + d >= n else o + d - r for o, d, n in zip(w0, wd, shape))
    assert all(h > l for l, h in zip(b0, b1)), "the case has no box at this radius"
    return b0, tuple(h - l for l, h in zip(b0, b1))


def _volumes(shape):
    """Named (volume, cut) pairs of ``shape``, read-only and made once."""
    if shape not in _CACHE:
        rng = np.random.default_rng(sum(shape))
        nz, ny, nx = shape
        corners = np.zeros(shape, dtype=U16)
        for z in (0, nz - 1):
            for y in (0, ny - 1):
                for x in (0, nx - 1):
                    corners[z, y, x] = 1000
        for x in (63, 64, 127, 128):                       # where the packed words of a row meet
            if x < nx:
                corners[nz // 2, ny // 2, x] = 1000
        dense = rng.integers(0, 2, shape).astype(U16) * 700
        sparse = (rng.random(shape) < 0.01).astype(U16) * 65535
        vols = {"corners": (corners, 1000), "half": (dense, 700), "all (cut 0)": (dense, 0), "none (cut 65536)": (dense, 65536),
                "sparse, cut 65535": (sparse, 65535), "no seed, cut 1": (np.zeros(shape, dtype=U16), 1)}
        for v, _ in vols.values():
            v.setflags(write=False)
        _CACHE[shape] = vols
    return _CACHE[shape]


def _run(ctx, vol, w0, wd, b0, bd, cut, radius, value=1, k=0, out_k=0, outs=("u16", "u8"), counts=None, zero_first=True,
         what=""):
    """One call in guarded, poisoned buffers, checked against the pyref; returns (mask of the box, (seeds, mask voxels)
    of the pyref)."""
    n = int(np.prod(bd))
    want, sums = ref.box_mask(vol, cut, radius, b0, bd, value)
    win = GuardedView(ctx, U16, int(np.prod(wd)), k=k, data=_window(vol, w0, wd))
    o16 = GuardedView(ctx, U16, n, k=out_k) if "u16" in outs else None
    o8 = GuardedView(ctx, np.uint8, n, k=out_k) if "u8" in outs else None
    own_counts = counts is None
    if own_counts:
        counts = GuardedView(ctx, np.uint64, 2)
    try:
        ctx.foreground_box_u16(win.ptr, vol.shape, w0, wd, b0, bd, cut, radius, value, o16.ptr if o16 else None,
                               o8.ptr if o8 else None, counts.ptr, zero_first=zero_first)
        ctx.sync()
        if o16:
            o16.check_output(want, f"{what}: out_u16")
        if o8:
            o8.check_output(want != 0, f"{what}: out_u8")
        if own_counts:
            counts.check_output(sums, f"{what}: counts")
        win.check_untouched(f"{what}: window")
    finally:
        for v in (win, o16, o8) + ((counts,) if own_counts else ()):
            if v is not None:
                v.free()
    return want, sums


# ---- the entry against the pyref: one box -----------------------------------------------------------------------------------
# (shape, window origin, window dims, element offset of the window's pointer, of the outputs' pointers)
SINGLE = {
    "A whole, pitch 27 (element loads)": (SHAPE_A, (0, 0, 0), (22, 19, 27), 0, 0),
    "A past the x face, pitch 32 (vector loads)": (SHAPE_A, (0, 0, 0), (22, 19, 32), 0, 0),
    "A past the x face, pointers + 1 element": (SHAPE_A, (0, 0, 0), (22, 19, 32), 1, 1),
    "A window at odd (1, 1, 3) to the faces, pitch 24": (SHAPE_A, (1, 1, 3), (21, 18, 24), 0, 0),
    "A window at odd (1, 1, 3) past the +x +y +z faces, pitch 32": (SHAPE_A, (1, 1, 3), (24, 20, 32), 0, 3),
    "A inner window (2, 1, 3), pitch 22 (element loads)": (SHAPE_A, (2, 1, 3), (18, 17, 22), 0, 0),
    "A inner window (2, 1, 2), pitch 24, pointer + 1": (SHAPE_A, (2, 1, 2), (18, 17, 24), 1, 0),
    "B whole, pitch 131 (element loads)": (SHAPE_B, (0, 0, 0), (9, 10, 131), 0, 0),
    "B past the faces, pitch 136 (vector loads)": (SHAPE_B, (0, 0, 0), (10, 12, 136), 0, 0),
    "B past the faces, pitch 136, pointers + 1 element": (SHAPE_B, (0, 0, 0), (10, 12, 136), 1, 1),
}


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_box(ctx, case, radius):
    shape, w0, wd, k, out_k = SINGLE[case]
    b0, bd = _box_of(shape, w0, wd, radius)
    past = any(o + d > n for o, d, n in zip(w0, wd, shape))
    for name, (vol, cut) in _volumes(shape).items():
        want, _ = _run(ctx, vol, w0, wd, b0, bd, cut, radius, value=1 if name == "half" else 40000, k=k, out_k=out_k,
                       what=f"{case}, {name}, radius {radius}")
        if past and name == "no seed, cut 1":
            # a kernel that trusted the 65535 past the faces would set the voxels at those faces: the pyref sets none
            assert not want.any()
        if past and name == "sparse, cut 65535":
            assert not want.all()


def test_each_output_alone(ctx):
    vol, cut = _volumes(SHAPE_A)["half"]
    for outs in (("u16",), ("u8",)):
        for wd, bd in (((22, 19, 32), (22, 19, 27)), ((22, 19, 32), (22, 19, 24))):     # element and vector stores
            _run(ctx, vol, (0, 0, 0), wd, (0, 0, 0), bd, cut, 2, value=9, outs=outs, what=f"{outs} alone, box {bd}")
    # the byte output at another phase of eight elements than the uint16 output: byte stores beside vector stores
    n = 22 * 19 * 24
    want, _ = ref.box_mask(vol, cut, 1, (0, 0, 0), (22, 19, 24), 5)
    win = GuardedView(ctx, U16, 22 * 19 * 32, data=_window(vol, (0, 0, 0), (22, 19, 32)))
    o16, o8 = GuardedView(ctx, U16, n), GuardedView(ctx, np.uint8, n, k=3)
    try:
        ctx.foreground_box_u16(win.ptr, SHAPE_A, (0, 0, 0), (22, 19, 32), (0, 0, 0), (22, 19, 24), cut, 1, 5, o16.ptr, o8.ptr)
        ctx.sync()
        o16.check_output(want, "both, phases differ: out_u16")
        o8.check_output(want != 0, "both, phases differ: out_u8")
    finally:
        for v in (win, o16, o8):
            v.free()


@pytest.mark.parametrize("radius", (1, 2, 3, 8))
def test_a_seed_in_the_halo_reaches_in_and_one_step_further_does_not(ctx, radius):
    shape = (30, 28, 40)
    b0, bd = (radius + 1, radius + 1, radius + 1), (30 - 2 * radius - 2, 28 - 2 * radius - 2, 40 - 2 * radius - 2)
    w0 = tuple(o - radius for o in b0)
    wd = tuple(d + 2 * radius for d in bd)
    probe = (b0[0], b0[1] + 2, b0[2] + 3)                                       # on the box's low z face
    t = (radius - 1) // 3
    split = (1 + t, t, radius - 1 - 2 * t)                                      # |split|_1 = radius, below the box in z
    for extra, reached in ((0, True), (1, False)):
        vol = np.zeros(shape, dtype=U16)
        seed = (probe[0] - split[0], probe[1] + split[1], probe[2] + split[2] + extra)     # L1 distance radius + extra
        assert seed[0] < b0[0], "the seed lies outside the box"
        vol[seed] = 500
        want, sums = _run(ctx, vol, w0, wd, b0, bd, 500, radius, value=2, what=f"seed at distance radius + {extra}")
        at = tuple(p - o for p, o in zip(probe, b0))
        assert bool(want[at]) == reached and sums[0] == 0 and (sums[1] > 0 or not reached)


@pytest.mark.parametrize("shape, radius", [((20, 18, 1000), 8), ((34, 33, 600), 1), ((34, 33, 600), 2)])
def test_more_than_one_region_along_every_axis(ctx, shape, radius):
    """A region gives 32 - 2 radius rows along z and y and 488 voxels along x."""
    rng = np.random.default_rng(3)
    vol = (rng.random(shape) < 0.002).astype(U16) * 300
    _run(ctx, vol, (0, 0, 0), shape, (0, 0, 0), shape, 300, radius, value=65535, what=f"{shape}, radius {radius}")


# ---- a partition with odd corners ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", (1, 3))
def test_partition(ctx, radius):
    vol, cut = _volumes(SHAPE_A)["sparse, cut 65535"]
    whole, totals = ref.box_mask(vol, cut, radius, (0, 0, 0), SHAPE_A, 1)
    boxes = measure_pyref.partition(SHAPE_A, ([7, 8], [9], [5, 13]))
    got = np.zeros(SHAPE_A, dtype=U16)
    counts = GuardedView(ctx, np.uint64, 2)
    try:
        for i, (b0, bd) in enumerate(boxes):
            w0 = tuple(max(0, o - radius) for o in b0)
            w1 = tuple(min(n, o + d + radius) for o, d, n in zip(b0, bd, SHAPE_A))
            part, _ = _run(ctx, vol, w0, tuple(h - l for l, h in zip(w0, w1)), b0, bd, cut, radius, counts=counts,
                           zero_first=i == 0, what=f"box {i}")
            got[tuple(slice(o, o + d) for o, d in zip(b0, bd))] = part
        ctx.sync()
        counts.check_output(totals, "the counts of the partition")
    finally:
        counts.free()
    np.testing.assert_array_equal(got, whole)
    assert totals[1] > totals[0] > 0


# ---- geometry and argument errors -----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    vol, cut = _volumes(SHAPE_A)["half"]
    b0, bd, r = (4, 4, 4), (10, 9, 12), 2
    w0, wd = (2, 2, 2), (14, 13, 16)
    win = GuardedView(ctx, U16, int(np.prod(wd)) + 8, data=np.zeros(int(np.prod(wd)) + 8, dtype=U16))
    o16, o8 = GuardedView(ctx, U16, int(np.prod(bd)) + 1), GuardedView(ctx, np.uint8, int(np.prod(bd)))
    counts = GuardedView(ctx, np.uint64, 2)

    def call(w0=w0, wd=wd, cut=cut, radius=r, value=1, p16=o16.ptr, p8=o8.ptr):
        ctx.foreground_box_u16(win.ptr, SHAPE_A, w0, wd, b0, bd, cut, radius, value, p16, p8, counts.ptr, zero_first=True)

    try:
        call()                                            # the geometry itself is accepted
        ctx.sync()
        for v in (o16, o8, counts):                       # poison them again
            v.buf.upload(v.host)
        bad = []
        for a in range(3):                                # a window missing one halo plane, on each side in turn
            low = list(w0)
            low[a] += 1
            short = list(wd)
            short[a] -= 1
            bad += [dict(w0=tuple(low), wd=tuple(short)), dict(wd=tuple(short))]
        bad += [dict(radius=9), dict(radius=-1), dict(cut=65537), dict(cut=-1), dict(value=0), dict(value=65536),
                dict(p16=None, p8=None), dict(p16=o16.ptr + 1)]
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        ctx.sync()
        for v in (o16, o8, counts, win):
            v.check_untouched("after the refused calls")
    finally:
        for v in (win, o16, o8, counts):
            v.free()


# ---- exabm4d_nonzero_u8_dev ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1))
def test_nonzero_u8(ctx, k):
    rng = np.random.default_rng(8)
    for n in (0, 1, 63, 64, 65, 1001):
        data = (rng.integers(0, 3, n) * rng.integers(1, 40000, n)).astype(U16)
        src = GuardedView(ctx, U16, n, k=k, data=data)
        dst = GuardedView(ctx, np.uint8, n, k=k)
        try:
            ctx.nonzero_u8(src.ptr, n, dst.ptr)
            ctx.sync()
            dst.check_output(data != 0, f"nonzero_u8 n={n} offset {k}")
            src.check_untouched(f"nonzero_u8 n={n}: src")
        finally:
            src.free()
            dst.free()


# ---- foreground_volume against the per-patch kernels ------------------------------------------------------------------------
def _tubes(shape, seed):
    """Poisson background with a few bright tubes along x."""
    rng = np.random.default_rng(seed)
    vol = rng.poisson(110, shape).astype(np.int64)
    for _ in range(4):
        z, y = rng.integers(2, shape[0] - 2), rng.integers(2, shape[1] - 2)
        vol[z:z + 2, y:y + 2, rng.integers(0, shape[2] // 2):] += rng.integers(400, 3000)
    return vol.astype(U16)


@pytest.mark.parametrize("name", ("tubes", "constant", "values 0..2"))
def test_foreground_volume_is_make_foreground_mask(name):
    shape = (24, 20, 40)
    vol = {"tubes": _tubes(shape, 1), "constant": np.full(shape, 777, dtype=U16),
           "values 0..2": np.random.default_rng(2).integers(0, 3, shape).astype(U16)}[name]
    for k, dilate in ((6, 1), (3, 2), (0, 0)):
        got = store_foreground.foreground_volume(vol, k, dilate)
        want = metrics.make_foreground_mask(vol, k, dilate)
        assert got.dtype == np.bool_ and got.shape == shape
        np.testing.assert_array_equal(got, want, err_msg=f"{name}, k={k}, dilate={dilate}")
    if name == "tubes":
        assert 0 < metrics.foreground_volume(vol, 6, 1).sum() < vol.size
        thr = float(np.median(vol)) + 50.0
        np.testing.assert_array_equal(store_foreground.foreground_volume(vol, threshold=thr, dilate=0), vol > thr)


# ---- foreground_store and recode_store against write_zarr, file for file ----------------------------------------------------
STORE_SHAPE, SRC_CHUNKS = (40, 36, 70), (1, 1, 16, 16, 32)
K, DILATE = 4, 2
BUDGETS = {"one brick": 4 << 30, "several bricks": 400_000, "one chunk per brick": 1}


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
    assert len(a) > 1
    for name in a:
        assert a[name] == b[name], f"{what}: {name} differs"


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """The source store, its pyref mask and the ``StoreMeasure`` of it, made once."""
    root = tmp_path_factory.mktemp("foreground_store")
    vol = _tubes(STORE_SHAPE, 7)
    nz, ny, nx = STORE_SHAPE
    for z, y, x in [(15, 3, 3), (3, 15, 40), (20, 20, 31), (7, 15, 63), (0, 0, 0), (nz - 1, ny - 1, nx - 1),
                    (0, ny - 1, 0), (nz - 1, 0, nx - 1)]:
        vol[z, y, x] = 60000                              # the last voxel of a brick along each axis; the corners
    vol.setflags(write=False)
    src = str(root / "src")
    chunk_store.write_zarr(vol, src, SRC_CHUNKS)
    mask = mask_pyref.fg_mask(vol, K, DILATE)
    assert 0 < mask.sum() < mask.size and mask[0, 0, 0] and mask[15, 3, 5] and mask[16, 3, 3]
    return {"root": root, "vol": vol, "src": src, "mask": mask, "measure": noise.measure_store(src),
            "thr": float(mask_pyref.fg_threshold(vol, K)), "ref": {}}


def _reference_mask_store(stored, chunks, value):
    key = (chunks, value)
    if key not in stored["ref"]:
        path = str(stored["root"] / ("ref_%d" % len(stored["ref"])))
        chunk_store.write_zarr((stored["mask"] * value).astype(U16), path, chunks or SRC_CHUNKS)
        stored["ref"][key] = path
    return stored["ref"][key]


@pytest.mark.parametrize("chunks", (None, (1, 1, 8, 16, 64)))
def test_foreground_store_is_write_zarr_of_the_whole_volume_mask(stored, chunks, tmp_path):
    n_fg = int(stored["mask"].sum())
    bricks = {}
    runs = [(b, "measure", 1) for b in BUDGETS] + [("several bricks", "none", 3), ("several bricks", "threshold", 1)]
    for budget, mode, value in runs:
        want = _reference_mask_store(stored, chunks, value)
        how = {"measure": dict(k=K, measure=stored["measure"]), "none": dict(k=K), "threshold": dict(threshold=stored["thr"])}[mode]
        st = {}
        dst = str(tmp_path / f"dst_{len(bricks)}_{mode}")
        res = store_foreground.foreground_store(stored["src"], dst, dilate=DILATE, value=value, chunks=chunks,
                                                budget_bytes=BUDGETS[budget], stats=st, **how)
        what = f"chunks {chunks}, {budget}, threshold from {mode}"
        _assert_same_store(dst, want, what)
        assert st["passes"] == (2 if mode == "none" else 1), what
        assert res["n_fg"] == n_fg and res["n"] == stored["vol"].size and res["fraction"] == n_fg / stored["vol"].size
        assert res["n_seed"] == int((stored["vol"].astype(np.float32) > np.float32(stored["thr"])).sum())
        assert res["cut"] == int(np.floor(stored["thr"])) + 1 and res["threshold"] == stored["thr"] and res["cratio"] > 1
        assert set(st["seconds"]) == {"measure", "read", "mask", "scatter", "encode", "files_write"}
        assert st["voxels_read"] >= stored["vol"].size and st["largest_alloc"] > 0
        if mode == "measure":
            bricks[budget] = st["bricks"]
    grid = [-(-s // c) for s, c in zip(STORE_SHAPE, (chunks or SRC_CHUNKS)[2:])]
    assert bricks["one brick"] == 1 < bricks["several bricks"] < bricks["one chunk per brick"] == int(np.prod(grid))


def test_the_mask_store_feeds_the_masked_measurements(stored, tmp_path):
    dst = str(tmp_path / "mask")
    res = metrics.foreground_store(stored["src"], dst, k=K, dilate=DILATE, measure=stored["measure"])
    m = noise.measure_store(stored["src"], mask=dst)
    assert int(m.counts_fg.sum()) == res["n_fg"] == int(stored["mask"].sum())
    np.testing.assert_array_equal(m.counts_fg, np.bincount(stored["vol"][stored["mask"]], minlength=65536))
    cmp = evaluate.compare_stores(stored["src"], stored["src"], mask=dst)
    assert cmp["n_fg"] == res["n_fg"] and cmp["lmax_fg"] == 0 and cmp["lmax_bg"] == 0


RECODE = {
    "exac, no mask": (lambda: ExacCodec(2), False, None),
    "block-bounded (16, 0)": (lambda: BlockBoundedCodec(16, 0), True, (16, 0)),
    "block-bounded from noise, k = 0.5": (lambda: BlockBoundedCodec.from_noise(
        {"gain": 1.0, "read_noise": 2.0, "offset": 100.0}, k=0.5, max_error=40, fg_max_error=1), True, (40, 1)),
}


@pytest.mark.parametrize("name", list(RECODE))
def test_recode_store_is_write_zarr_under_the_mask(stored, name, tmp_path):
    make, with_mask, bounds = RECODE[name]
    mask_store = _reference_mask_store(stored, None, 1) if with_mask else None
    want = str(tmp_path / "want")
    ratio = chunk_store.write_zarr(stored["vol"], want, SRC_CHUNKS, codec=make(), mask=stored["mask"] if with_mask else None)
    bricks = []
    for budget in ("one brick", "several bricks"):
        st = {}
        dst = str(tmp_path / f"dst_{len(bricks)}")
        got = chunk_store.recode_store(stored["src"], dst, codec=make(), mask=mask_store, budget_bytes=BUDGETS[budget], stats=st)
        _assert_same_store(dst, want, f"{name}, {budget}")
        assert got == ratio
        bricks.append(st["bricks"])
    assert bricks[0] == 1 < bricks[1]
    if bounds:
        cmp = evaluate.compare_stores(stored["src"], dst, mask=mask_store)
        assert cmp["lmax_fg"] <= bounds[1] and cmp["lmax_bg"] <= bounds[0], (cmp["lmax_fg"], cmp["lmax_bg"])
        assert cmp["n_fg"] == int(stored["mask"].sum())
