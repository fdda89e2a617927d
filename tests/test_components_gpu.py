"""Connected components of the seeds of a window on the GPU: ``exabm4d_component_seeds_u16_dev`` and
``exabm4d_label_components_dev`` in guarded, poisoned buffers against the pyref, bit for bit, and the mask functions and
``foreground_store`` with ``min_voxels`` against ``write_zarr`` of the pyref mask, file for file."""
import os

import numpy as np
import pytest

import components_pyref as cref
from util import GuardedView

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning import metrics
from aind_exaspim_image_compression.utils import chunk_store, store_foreground

pytestmark = pytest.mark.gpu
U16, U32 = np.uint16, np.uint32
CUT = 1000
TZ, TY, TX = _native.CC_TILE
SHAPE_A, SHAPE_B, SHAPE_T = (22, 19, 27), (9, 10, 131), (TZ + 1, TY + 1, TX + 1)
CONNECTIVITIES = (6, 26)
_CACHE = {}


def _window(vol, origin, dims):
    """The window ``origin + [0, dims)`` of ``vol``; what lies past the volume's faces holds 65535."""
    out = np.full(dims, 65535, dtype=U16)
    inside = tuple(slice(0, min(d, n - o)) for o, d, n in zip(origin, dims, vol.shape))
    out[inside] = vol[tuple(slice(o, o + s.stop) for o, s in zip(origin, inside))]
    return out


def _box_of(shape, w0, wd, r):
    """The largest box whose growth by ``r``, cut at the volume, the window holds; None if there is none."""
    b0 = tuple(0 if o == 0 else o + r for o in w0)
    b1 = tuple(n if o + d >= n else o + d - r for o, d, n in zip(w0, wd, shape))
    return (b0, tuple(h - l for l, h in zip(b0, b1))) if all(h > l for l, h in zip(b0, b1)) else None


def _serpentine(shape):
    """One path through the whole volume: every other row of every other plane, joined at alternating ends."""
    nz, ny, nx = shape
    plane = np.zeros((ny, nx), dtype=bool)
    plane[::2] = True
    for j, y in enumerate(range(1, ny, 2)):
        if y + 1 < ny:
            plane[y, nx - 1 if j % 2 == 0 else 0] = True
    last = ny - 1 - (ny - 1) % 2                          # the row the plane's path ends in, and the end it ends at
    ends = [(0, 0), (last, nx - 1 if (last // 2) % 2 == 0 else 0)]
    s = np.zeros(shape, dtype=bool)
    s[::2] = plane
    for j, z in enumerate(range(1, nz, 2)):
        if z + 1 < nz:
            s[z][ends[(j + 1) % 2]] = True
    return s


def _nested_u(shape):
    """In every other plane, U shapes inside each other, open towards x = 0: two arms that meet only at the far end."""
    nz, ny, nx = shape
    plane = np.zeros((ny, nx), dtype=bool)
    for k in range(0, min(ny // 2, nx - 1), 2):
        if ny - 1 - k - k < 2:
            break
        plane[k, :nx - k] = plane[ny - 1 - k, :nx - k] = True
        plane[k:ny - k, nx - 1 - k] = True
    s = np.zeros(shape, dtype=bool)
    s[::2] = plane
    return s


def _patterns(shape):
    """Named boolean seed patterns of ``shape``, read-only and made once."""
    if shape not in _CACHE:
        rng = np.random.default_rng(sum(shape))
        nz, ny, nx = shape
        z, y, x = np.indices(shape)
        pats = {"empty": np.zeros(shape, dtype=bool), "full": np.ones(shape, dtype=bool)}
        for d in (0.05, 0.2, 0.5):
            pats[f"random {d}"] = rng.random(shape) < d
        pats["checkerboard"] = (z + y + x) % 2 == 0
        pats["space diagonal"] = (z == y) & (y == x)
        pats["serpentine"] = _serpentine(shape)
        pats["nested U"] = _nested_u(shape)
        pairs = np.zeros(shape, dtype=bool)                # pairs that touch through a tile corner, an edge, a face
        for a, b in [((TZ - 1, TY - 1, TX - 1), (TZ, TY, TX)), ((TZ - 1, TY, 31), (TZ, TY - 1, 30)),
                     ((TZ - 1, TY - 1, 5), (TZ, TY, 5)), ((TZ - 1, 3, 9), (TZ, 3, 9)), ((2, TY - 1, 12), (2, TY, 13)),
                     ((4, 2, TX - 1), (5, 3, TX)), ((4, 5, TX - 1), (4, 5, TX))]:
            if all(i < n for i, n in zip(b, shape)):
                pairs[a] = pairs[b] = True
        pats["pairs across tiles"] = pairs
        corners = np.zeros(shape, dtype=bool)
        for cz in (0, nz - 1):
            for cy in (0, ny - 1):
                for cx in (0, nx - 1):
                    corners[cz, cy, cx] = True
        for cx in (63, 64, 127, 128):
            if cx < nx:
                corners[nz // 2, ny // 2, cx] = True
        pats["corners and x = 63, 64, 127, 128"] = corners
        planted = rng.random(shape) < 0.01                 # a component of exactly PLANTED voxels, alone
        planted[1:6, 1:6, 1:11] = False
        planted[3, 3, 2:2 + PLANTED] = True
        pats["planted"] = planted
        for p in pats.values():
            p.setflags(write=False)
        _CACHE[shape] = pats
    return _CACHE[shape]


PLANTED = 5


def _volume(seeds):
    """uint16 counts: >= CUT exactly at the seeds, something below elsewhere."""
    rng = np.random.default_rng(int(seeds.sum()))
    low = rng.integers(0, CUT, seeds.shape)
    high = rng.integers(CUT, 65536, seeds.shape)
    return np.where(seeds, high, low).astype(U16)


def _count_box(b0, bd):
    """A sub-box of the box: without its first layer along z and its last voxels along x where it has more than one."""
    c0 = (b0[0] + (1 if bd[0] > 1 else 0), b0[1], b0[2])
    cd = (bd[0] - (1 if bd[0] > 1 else 0), bd[1], bd[2] - (1 if bd[2] > 1 else 0))
    return c0, cd


def _run(ctx, vol, w0, wd, b0, bd, min_voxels, connectivity, k=0, out_k=0, what=""):
    """Two calls in guarded, poisoned buffers (the second without zeroing the counters), each checked against the
    pyref: labels, sizes, filtered seeds, counters; the window is left as it was."""
    c0, cd = _count_box(b0, bd)
    want = cref.component_seeds(vol, CUT, min_voxels, connectivity, b0, bd, c0, cd)
    _, rd = _native.components_region(vol.shape, b0, bd, min_voxels)
    assert rd == want["labels"].shape
    nr, nb = int(np.prod(rd)), int(np.prod(bd))
    win = GuardedView(ctx, U16, int(np.prod(wd)), k=k, data=_window(vol, w0, wd))
    seeds = GuardedView(ctx, U16, nb, k=out_k)
    labels, sizes = GuardedView(ctx, U32, nr, k=out_k), GuardedView(ctx, U32, nr)
    counts = GuardedView(ctx, np.uint64, 3)
    scratch = GuardedView(ctx, U32, _native.components_scratch_bytes(wd, connectivity) // 4)
    views = (win, seeds, labels, sizes, counts, scratch)
    try:
        for launch in (1, 2):
            ctx.component_seeds_u16(win.ptr, vol.shape, w0, wd, b0, bd, CUT, min_voxels, connectivity, count_origin=c0,
                                    count_dims=cd, seeds_u16=seeds.ptr, labels=labels.ptr, sizes=sizes.ptr,
                                    scratch=scratch.ptr, scratch_bytes=4 * scratch.n, counts=counts.ptr,
                                    zero_first=launch == 1)
            ctx.sync()
            labels.check_output(want["labels"], f"{what}, launch {launch}: labels")
            sizes.check_output(want["sizes"], f"{what}, launch {launch}: sizes")
            seeds.check_output(want["seeds_u16"], f"{what}, launch {launch}: seeds_u16")
            counts.check_output([launch * c for c in want["counts"]], f"{what}, launch {launch}: counts")
            win.check_untouched(f"{what}: window")
            got = scratch._download()                      # the scratch is the call's to write, the bytes around it not
            np.testing.assert_array_equal(got[:scratch.lo], scratch.host[:scratch.lo], err_msg=f"{what}: before scratch")
            np.testing.assert_array_equal(got[scratch.hi:], scratch.host[scratch.hi:], err_msg=f"{what}: after scratch")
    finally:
        for v in views:
            v.free()
    return want


# ---- the windowed entry against the pyref -------------------------------------------------------------------------------------
# (shape, window origin, window dims, element offset of the window's pointer, of the outputs' pointers): the alignments of
# test_store_foreground_gpu.SINGLE, and the shape of one voxel more than a tile
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
    "T whole: a tile and one voxel on every axis": (SHAPE_T, (0, 0, 0), SHAPE_T, 0, 0),
    "T past the faces, pitch 72, pointers + 1 element": (SHAPE_T, (0, 0, 0), (TZ + 2, TY + 3, TX + 8), 1, 1),
}
WHOLE = [c for c in SINGLE if " whole" in c]
RUNS = [(c, m) for c in SINGLE for m in (1, 3)] + [(c, m) for c in WHOLE for m in (2, PLANTED, PLANTED + 1, 64)]
assert all(_box_of(SINGLE[c][0], SINGLE[c][1], SINGLE[c][2], m - 1) for c, m in RUNS)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("case, min_voxels", RUNS)
def test_component_seeds_of_a_window(ctx, case, min_voxels, connectivity):
    shape, w0, wd, k, out_k = SINGLE[case]
    b0, bd = _box_of(shape, w0, wd, min_voxels - 1)
    for name, seeds in _patterns(shape).items():
        want = _run(ctx, _volume(seeds), w0, wd, b0, bd, min_voxels, connectivity, k=k, out_k=out_k,
                    what=f"{case}, {name}, min_voxels {min_voxels}, connectivity {connectivity}")
        if case in WHOLE:                                  # the patterns are what their names say
            n = cref.count_components(want["labels"])
            if name in ("checkerboard", "space diagonal"):
                assert n == (int(seeds.sum()) if connectivity == 6 else 1)
            if name in ("serpentine", "full"):
                assert n == 1
            if name == "planted":
                assert want["sizes"][3, 3, 2] == PLANTED and want["seeds_u16"][3, 3, 2] == (min_voxels <= PLANTED)
            if name == "pairs across tiles" and shape != SHAPE_A:
                assert n < int(seeds.sum()) and (connectivity == 26) == (n * 2 == int(seeds.sum()))


def test_padding_past_the_faces_neither_seeds_nor_connects(ctx):
    """Two seeds at the +x face, two rows apart: the 65535 of the padding beside them would join them."""
    seeds = np.zeros(SHAPE_A, dtype=bool)
    seeds[5, 5, -1] = seeds[5, 7, -1] = seeds[-1, -1, -1] = True
    want = _run(ctx, _volume(seeds), (0, 0, 0), (24, 20, 32), (0, 0, 0), SHAPE_A, 2, 26, what="padding")
    assert cref.count_components(want["labels"]) == 3 and not want["seeds_u16"].any()


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    b0, bd, w0, wd, m = (4, 4, 4), (10, 9, 12), (2, 2, 2), (14, 13, 16), 3
    nr = int(np.prod(wd))
    win = GuardedView(ctx, U16, nr, data=np.zeros(nr, dtype=U16))
    seeds, labels, sizes = GuardedView(ctx, U16, int(np.prod(bd))), GuardedView(ctx, U32, nr), GuardedView(ctx, U32, nr)
    counts = GuardedView(ctx, np.uint64, 3)
    scratch = GuardedView(ctx, U32, _native.components_scratch_bytes(wd) // 4)
    views = (win, seeds, labels, sizes, counts, scratch)

    def call(w0=w0, wd=wd, min_voxels=m, connectivity=26, cut=CUT, c0=b0, cd=bd, labels_ptr=labels.ptr,
             scratch_ptr=scratch.ptr, scratch_bytes=4 * scratch.n):
        ctx.component_seeds_u16(win.ptr, SHAPE_A, w0, wd, b0, bd, cut, min_voxels, connectivity, count_origin=c0,
                                count_dims=cd, seeds_u16=seeds.ptr, labels=labels_ptr, sizes=sizes.ptr, scratch=scratch_ptr,
                                scratch_bytes=scratch_bytes, counts=counts.ptr, zero_first=True)

    try:
        call()                                            # the geometry itself is accepted
        ctx.sync()
        for v in views:                                   # poison them again
            v.buf.upload(v.host)
        bad = []
        for a in range(3):                                # a window missing one halo plane, on each side in turn
            low, short = list(w0), list(wd)
            low[a] += 1
            short[a] -= 1
            bad += [dict(w0=tuple(low), wd=tuple(short)), dict(wd=tuple(short))]
        bad += [dict(min_voxels=0), dict(min_voxels=4), dict(connectivity=18), dict(connectivity=8), dict(cut=65537),
                dict(cut=-1), dict(c0=(3, 4, 4)), dict(cd=(10, 9, 13)), dict(labels_ptr=labels.ptr + 2),
                dict(scratch_ptr=scratch.ptr + 1), dict(scratch_ptr=0), dict(scratch_bytes=4 * scratch.n - 1024)]
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        ctx.sync()
        for v in views:
            v.check_untouched("after the refused calls")
    finally:
        for v in views:
            v.free()


# ---- the resident entry and the functions of metrics --------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", (SHAPE_B, SHAPE_T))
def test_label_components_and_remove_small_components(shape, connectivity):
    for name, seeds in _patterns(shape).items():
        what = f"{name}, connectivity {connectivity}"
        lab = cref.labels(seeds, connectivity)
        got, n = metrics.label_components(seeds, connectivity)
        assert got.dtype == np.int32 and n == cref.count_components(lab), what
        np.testing.assert_array_equal(got, lab.astype(np.int32), err_msg=what)
        if name in ("random 0.05", "random 0.2", "planted", "nested U"):
            re, n_re = metrics.label_components(seeds.astype(U16) * 7, connectivity, relabel=True)
            want_re, want_n = cref.relabel(lab)
            assert n_re == want_n == n and re.dtype == np.int32
            np.testing.assert_array_equal(re, want_re, err_msg=what)
            for m in (1, 2, PLANTED, PLANTED + 1, 64, 1000):
                keep = metrics.remove_small_components(seeds, m, connectivity)
                assert keep.dtype == np.bool_
                np.testing.assert_array_equal(keep, cref.kept(seeds, m, connectivity), err_msg=f"{what}, min_voxels {m}")


def test_label_components_of_a_resident_uint16_array(ctx):
    seeds = _patterns(SHAPE_B)["random 0.2"]
    vol = _volume(seeds)
    want = cref.component_seeds(vol, CUT, 4, 6, (0, 0, 0), SHAPE_B)
    src = GuardedView(ctx, U16, vol.size, k=1, data=vol)
    labels, sizes = GuardedView(ctx, U32, vol.size), GuardedView(ctx, U32, vol.size)
    kept, counts = GuardedView(ctx, np.uint8, vol.size, k=3), GuardedView(ctx, np.uint64, 3)
    try:
        ctx.label_components(src.ptr, U16, SHAPE_B, cut=CUT, min_voxels=4, connectivity=6, labels=labels.ptr,
                             sizes=sizes.ptr, kept_u8=kept.ptr, counts=counts.ptr)
        ctx.sync()
        labels.check_output(want["labels"], "labels")
        sizes.check_output(want["sizes"], "sizes")
        kept.check_output(want["seeds_u16"], "kept_u8")
        counts.check_output(want["counts"], "counts")
        src.check_untouched("src")
    finally:
        for v in (src, labels, sizes, kept, counts):
            v.free()


def _hot_tubes(shape, seed, faces):
    """Poisson background, bright tubes along x, hot pixels, and straight components of 1..9 voxels across ``faces``."""
    rng = np.random.default_rng(seed)
    vol = rng.poisson(110, shape).astype(np.int64)
    for _ in range(4):
        z, y = rng.integers(2, shape[0] - 2), rng.integers(2, shape[1] - 2)
        vol[z:z + 2, y:y + 2, rng.integers(0, shape[2] // 2):] += rng.integers(400, 3000)
    vol[rng.random(shape) < 0.004] = 60000
    for axis, at in faces:
        for j, length in enumerate(range(1, 10)):
            p = [2 + 3 * j, 3 + 3 * j, 4 + 5 * j]
            for t in range(length):
                p[axis] = at - (length + 1) // 2 + t
                if all(0 <= c < n for c, n in zip(p, shape)):
                    vol[tuple(p)] = 50000
    for c in [(0, 0, 0), tuple(n - 1 for n in shape)]:
        vol[c] = 60000
    return vol.astype(U16)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_the_in_memory_masks_filter_before_they_dilate(connectivity):
    import mask_pyref
    shape = (24, 20, 70)
    vol = _hot_tubes(shape, 3, [(0, 8), (1, 8), (2, 64)])
    vol.setflags(write=False)
    for k, dilate, m in ((6, 1, 2), (4, 2, 4), (6, 0, 9), (6, 3, 200)):
        thr = float(mask_pyref.fg_threshold(vol, k))
        seeds = vol.astype(np.float32) > np.float32(thr)
        want = cref.filtered_mask(seeds, m, connectivity, dilate)
        assert want.sum() < cref.filtered_mask(seeds, 0, connectivity, dilate).sum()          # the filter removes something
        what = f"k {k}, dilate {dilate}, min_voxels {m}, connectivity {connectivity}"
        got = store_foreground.foreground_volume(vol, k, dilate, min_voxels=m, connectivity=connectivity)
        np.testing.assert_array_equal(got, want, err_msg="foreground_volume: " + what)
        got = store_foreground.foreground_volume(vol, threshold=thr, dilate=dilate, min_voxels=m, connectivity=connectivity)
        np.testing.assert_array_equal(got, want, err_msg="foreground_volume, threshold: " + what)
        got = metrics.make_foreground_mask(vol, k, dilate, min_voxels=m, connectivity=connectivity)
        assert got.dtype == np.bool_
        np.testing.assert_array_equal(got, want, err_msg="make_foreground_mask: " + what)
    np.testing.assert_array_equal(metrics.make_foreground_mask(vol, 6, 1, min_voxels=0), metrics.make_foreground_mask(vol, 6, 1))
    np.testing.assert_array_equal(store_foreground.foreground_volume(vol, 6, 1, min_voxels=0),
                                  store_foreground.foreground_volume(vol, 6, 1))


# ---- foreground_store with min_voxels against write_zarr, file for file ----------------------------------------------------------
STORE_SHAPE, SRC_CHUNKS, DST_CHUNKS = (40, 36, 70), (1, 1, 16, 16, 32), (1, 1, 7, 9, 33)
THR, DILATE = 300.0, 2
BUDGETS = {"one brick": 4 << 30, "several bricks": 1_200_000, "one chunk per brick": 1}


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
    """The source store, made once: components of 1..9 voxels straddle the faces of the bricks the budgets give."""
    root = tmp_path_factory.mktemp("components_store")
    vol = _hot_tubes(STORE_SHAPE, 7, [(0, 21), (0, 28), (1, 18), (1, 27), (2, 33)])
    vol.setflags(write=False)
    src = str(root / "src")
    chunk_store.write_zarr(vol, src, SRC_CHUNKS)
    return {"root": root, "vol": vol, "src": src}


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("min_voxels", (2, 9))
def test_foreground_store_with_min_voxels_is_write_zarr_of_the_filtered_mask(stored, min_voxels, connectivity, tmp_path):
    vol = stored["vol"]
    seeds = vol > THR
    keep = cref.kept(seeds, min_voxels, connectivity)
    mask = cref.filtered_mask(seeds, min_voxels, connectivity, DILATE)
    comp = cref.sizes(cref.labels(seeds, connectivity))
    n_dropped = int(((comp > 0) & (comp < min_voxels)).sum())
    assert 0 < keep.sum() < seeds.sum() and n_dropped > 0
    want = str(tmp_path / "want")
    chunk_store.write_zarr((mask * 3).astype(U16), want, DST_CHUNKS)
    n_chunks = int(np.prod([-(-s // c) for s, c in zip(STORE_SHAPE, DST_CHUNKS[2:])]))
    bricks = {}
    for budget in BUDGETS:
        st = {}
        dst = str(tmp_path / f"dst_{len(bricks)}")
        res = store_foreground.foreground_store(stored["src"], dst, threshold=THR, dilate=DILATE, value=3, chunks=DST_CHUNKS,
                                                budget_bytes=BUDGETS[budget], stats=st, min_voxels=min_voxels,
                                                connectivity=connectivity)
        what = f"min_voxels {min_voxels}, connectivity {connectivity}, {budget}"
        _assert_same_store(dst, want, what)
        assert (res["n_seed"], res["n_kept"], res["n_dropped_components"], res["n_fg"]) == \
            (int(seeds.sum()), int(keep.sum()), n_dropped, int(mask.sum())), what
        assert res["n"] == vol.size and res["fraction"] == int(mask.sum()) / vol.size
        assert st["voxels_read"] >= vol.size and st["largest_alloc"] > 0
        if st["bricks"] < n_chunks:                       # bricks of more than one chunk keep to the budget
            assert st["largest_alloc"] <= BUDGETS[budget], what
        bricks[budget] = st["bricks"]
    assert bricks["one brick"] == 1 < bricks["several bricks"] < bricks["one chunk per brick"] == n_chunks


def test_foreground_store_with_min_voxels_0_writes_what_it_wrote_before(stored, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    kw = dict(threshold=THR, dilate=DILATE, chunks=DST_CHUNKS, budget_bytes=BUDGETS["several bricks"])
    res_a = store_foreground.foreground_store(stored["src"], a, **kw)
    res_b = store_foreground.foreground_store(stored["src"], b, min_voxels=0, connectivity=6, **kw)
    _assert_same_store(a, b, "min_voxels 0")
    assert res_a == res_b and res_a["n_kept"] == res_a["n_seed"] and res_a["n_dropped_components"] == 0
