"""The host side of ``inference.predict_store`` without a GPU: ``store_predict.plan_predict`` against
brute force, the numpy yardstick ``stitch_pyref`` against results recorded from the reference's ``predict``, and
``predict_store``'s argument errors, which must come before any device context exists."""
import itertools
import os

import numpy as np
import pytest

import stitch_pyref
from oracle.host_oracle import TransformOracle
from test_oracle_golden import TRANSFORM_CFGS

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.utils import store_predict
from aind_exaspim_image_compression.utils.store_predict import plan_predict

SHAPES = [(45, 38, 52), (20, 18, 6), (130, 64, 70)]
CHUNKS = [(4, 16, 16), (8, 8, 8), (32, 32, 32)]
GEOMETRIES = [(16, 6, 2), (64, 12, 5)]             # (patch, overlap, trim)
BUDGETS = [1, 150_000, 600_000, 3 << 20, 7 << 20, 1 << 62]
BATCH = 2


def _one_chunk(brick, chunk):
    return all(e <= c for e, c in zip(brick.extent, chunk))


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_plan_predict_by_brute_force(shape, chunk, geometry):
    patch, overlap, trim = geometry
    stride, core = patch - overlap, patch - 2 * trim
    starts = stitch_pyref.patch_starts(shape, patch, overlap)
    unique = inference.count_patches(inference._ShapeOnly((1, 1) + shape), patch, overlap)
    assert len(starts) == unique == int(np.prod([store_predict.axis_patches(n, patch, overlap) for n in shape]))
    n_chunks = int(np.prod([-(-s // c) for s, c in zip(shape, chunk)]))
    counts = []
    for budget in BUDGETS:
        bricks = plan_predict(shape, chunk, patch, overlap, trim, BATCH, budget)
        assert bricks == plan_predict(shape, chunk, patch, overlap, trim, BATCH, budget)       # deterministic
        counts.append(len(bricks))
        assert [b.origin for b in bricks] == sorted(b.origin for b in bricks)                  # raster order
        owner = np.zeros(shape, dtype=np.int32)
        needed = set()
        for b in bricks:
            lo, hi = b.origin, tuple(o + e for o, e in zip(b.origin, b.extent))
            owner[tuple(slice(a, z) for a, z in zip(lo, hi))] += 1
            for a in range(3):                         # faces on the chunk grid or on the volume's face
                assert lo[a] % chunk[a] == 0 and (hi[a] % chunk[a] == 0 or hi[a] == shape[a])
                assert 0 <= lo[a] < hi[a] <= shape[a]
            # the patches whose cores meet the brick, by brute force over every patch of the volume
            want = {s for s in starts
                    if all(max(s[a] + trim, lo[a]) < min(s[a] + trim + core, shape[a], hi[a]) for a in range(3))}
            got = {tuple((b.first[a] + i[a]) * stride for a in range(3))
                   for i in itertools.product(*(range(c) for c in b.count))}
            assert got == want and len(got) == b.n_patches
            needed |= got
            # the window: every voxel of those patches inside the volume and nothing else (per axis: the patch set is
            # a product, as just checked)
            for a in range(3):
                cover = {v for s in want for v in range(s[a], min(s[a] + patch, shape[a]))}
                assert cover == set(range(b.win_origin[a], b.win_origin[a] + b.win_extent[a]))
            pv = patch ** 3
            slabs, slab = store_predict.window_slabs(b.win_extent[0], chunk[0])     # the window as it is held
            assert slabs * slab >= b.win_extent[0] and (slabs == 0 or slabs * slab - b.win_extent[0] < slabs)
            cost = (2 * slabs * slab * b.win_extent[1] * b.win_extent[2] + 4 * pv * b.n_patches + 4 * pv * BATCH +
                    (2 + 8) * int(np.prod(b.extent)) + budget // 8)
            assert b.cost == cost
            assert cost <= budget or _one_chunk(b, chunk)
        assert np.all(owner == 1)                      # the bricks partition the volume
        assert needed == set(starts)                   # every patch of the whole-volume call runs somewhere
    assert counts[0] == n_chunks and counts[-1] == 1   # one chunk a brick ... the whole volume
    assert counts == sorted(counts, reverse=True)      # a larger budget never gives more bricks


def test_plan_predict_grows_bricks_between_one_chunk_and_the_volume():
    bricks = plan_predict((45, 38, 52), (4, 16, 16), 16, 6, 2, BATCH, 600_000)
    assert 1 < len(bricks) < 12 * 3 * 4
    ext = bricks[0].extent                             # as cubic as chunks of (4, 16, 16) allow
    assert max(ext) - min(ext) <= 16


def test_facts_fixed_by_hand():
    shape, (patch, overlap, trim) = (45, 38, 52), (16, 6, 2)
    assert [store_predict.axis_patches(n, patch, overlap) for n in shape] == [4, 4, 5]
    covered = np.zeros(45, bool)
    for i in range(4):
        covered[i * 10 + 2:i * 10 + 2 + 12] = True
    assert [z for z in range(45) if not covered[z]] == [0, 1, 44]
    for z in range(45):
        assert (store_predict.patch_range(z, z + 1, 45, patch, overlap, trim)[1] > 0) == covered[z]
    bricks = plan_predict(shape, (4, 16, 16), patch, overlap, trim, BATCH, 1)
    last = [b for b in bricks if b.origin[0] == 44]
    assert len(last) == 3 * 4 and all(b.extent[0] == 1 and b.count[0] == 0 and b.n_patches == 0 for b in last)
    assert all(b.win_extent == (0, 0, 0) for b in last)
    # x <= overlap: no patch at all
    assert store_predict.axis_patches(6, patch, overlap) == 0
    assert all(b.n_patches == 0 for b in plan_predict((20, 18, 6), (8, 8, 8), patch, overlap, trim, BATCH, 1 << 62))
    assert inference.count_patches(inference._ShapeOnly((1, 1, 20, 18, 6)), patch, overlap) == 0


def test_plan_predict_rejects_bad_arguments():
    for bad in [dict(shape=(0, 4, 4)), dict(chunks_zyx=(4, 4)), dict(patch_size=16, overlap=16), dict(trim=8),
                dict(batch_size=0), dict(budget_bytes=0)]:
        args = dict(shape=(45, 38, 52), chunks_zyx=(4, 16, 16), patch_size=16, overlap=6, trim=2, batch_size=2,
                    budget_bytes=1 << 20)
        args.update(bad)
        with pytest.raises(ValueError):
            plan_predict(**args)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch.npz")
# tests/golden/make_stitch_golden.py: name -> (shape, patch, overlap, trim, seed)
GOLDEN_CASES = {"a": ((27, 24, 33), 16, 6, 2, 21), "b": ((30, 17, 33), 16, 10, 1, 22)}


@pytest.mark.parametrize("name", ["anscombe_g8_rn5_o100", "linear_35_1000_8"])
@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_stitch_pyref_is_the_reference_predict(case, name):
    """What the reference's own ``predict`` returned for seeded predictions (a model that ignores its input), and
    for case "a" what that model was fed: recorded results, compared bit for bit."""
    shape, patch, overlap, trim, seed = GOLDEN_CASES[case]
    gold = np.load(GOLDEN)
    starts = stitch_pyref.patch_starts(shape, patch, overlap)
    preds = stitch_pyref.random_predictions(len(starts), patch, seed)
    assert np.signbit(preds[preds == 0]).all() and (preds < 0).any()
    got = stitch_pyref.stitch(preds, starts, shape, trim, TRANSFORM_CFGS[name])
    np.testing.assert_array_equal(got, gold[f"{case}/{name}/predict"])
    assert got.dtype == np.uint16 and len(np.unique(got)) > 100
    if case == "a":
        vol = (np.random.default_rng(seed).integers(0, 16, shape) * 70).astype(np.uint16)
        np.testing.assert_array_equal(stitch_pyref.gather_patches(vol, TRANSFORM_CFGS[name], patch, starts),
                                      gold[f"{case}/{name}/inputs"])


def test_gather_pyref_pads_with_zeros_after_the_transform():
    cfg = TRANSFORM_CFGS["asinh_s32_o35"]
    counts = np.full((20, 20, 20), 500, np.uint16)
    got = stitch_pyref.gather_patches(counts, cfg, 16, [(10, 0, 10)])
    inside = TransformOracle(cfg).forward(counts[:1, :1, :1])[0, 0, 0]
    assert inside != 0 and TransformOracle(cfg).forward(np.zeros(1, np.uint16))[0] != 0
    assert np.all(got[0, :10, :, :10] == inside) and np.all(got[0, 10:] == 0) and np.all(got[0, :, :, 10:] == 0)


class _Int32Store:
    dtype = np.dtype(np.int32)
    shape, chunks, device, max_pool_bytes = (1, 1, 8, 8, 8), (1, 1, 8, 8, 8), None, 1 << 30

    def read_patches(self, *a, **k):
        raise AssertionError("nothing may be read")


class _OtherDeviceStore(_Int32Store):
    """A uint16 source opened for cuda:1, where the model (a callable: cuda:0) and ``device=0`` do not run."""
    dtype, device = np.dtype(np.uint16), 1


@pytest.mark.parametrize("bad", [
    dict(precision="fp8"), dict(batch_size=0), dict(patch_size=16, overlap=16), dict(patch_size=16, trim=8),
    dict(budget_bytes=0), dict(chunks=(4, 16, 16)), dict(chunks=(1, 2, 4, 16, 16)), dict(chunks=(1, 1, 0, 16, 16)),
    dict(src=_Int32Store()), dict(src=_OtherDeviceStore()), dict(src=_OtherDeviceStore(), device=0),
])
def test_predict_store_argument_errors_come_before_any_context(bad, tmp_path, monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a device context was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "context", no_context)
    monkeypatch.setattr(_native, "Context", no_context)
    args = dict(src=str(tmp_path / "no-such-store"), dst_path=str(tmp_path / "dst"), model=lambda x: x,
                transform=None, verbose=False)
    args.update(bad)
    with pytest.raises(ValueError):
        inference.predict_store(**args)
    assert not (tmp_path / "dst").exists()
