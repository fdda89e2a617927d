"""The numpy restatement of a label pyramid level (tests/label_pyramid_pyref.py) against a triple loop
with ``collections.Counter`` over Python integers (CPU)."""
import collections
import itertools

import numpy as np
import pytest

import label_pyramid_pyref as ref

FACTORS = [f for f in itertools.product((1, 2), repeat=3) if max(f) == 2]
BIG_IDS = [1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1]


def loop_level(vol, factors, edge, zeros):
    nz, ny, nx = vol.shape
    level = ref.level_shape(vol.shape, factors, edge)
    out = np.zeros(level, dtype=vol.dtype)
    for z, y, x in itertools.product(*(range(n) for n in level)):
        sl = tuple(slice(i * f, min(n, (i + 1) * f)) for i, f, n in zip((z, y, x), factors, (nz, ny, nx)))
        present = [int(v) for v in vol[sl].reshape(-1)]
        assert present
        if zeros == "ignore":
            present = [v for v in present if v != 0]
        if not present:
            continue
        counts = collections.Counter(present)
        most = max(counts.values())
        out[z, y, x] = min(v for v, c in counts.items() if c == most)
    return out


def volumes():
    rng = np.random.default_rng(11)
    out = []
    for shape in ((5, 6, 7), (4, 4, 4)):
        for alphabet in ([0, 7], [0, 3, 9], [5, 6, 2 ** 31]):
            out.append(("u32 %s %s" % (shape, alphabet), rng.choice(np.array(alphabet, dtype=np.uint32), size=shape)))
        for alphabet in ([0, 2 ** 63], [0, 2 ** 32, 2 ** 32 + 1], [2 ** 32 - 1, 2 ** 64 - 1, 1]):
            out.append(("u64 %s %s" % (shape, alphabet), rng.choice(np.array(alphabet, dtype=np.uint64), size=shape)))
        out.append(("u64 %s ids" % (shape,), rng.choice(np.array([0] + BIG_IDS, dtype=np.uint64), size=shape)))
    return out


VOLUMES = volumes()


@pytest.mark.parametrize("zeros", ref.ZEROS)
@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("factors", FACTORS)
def test_restatement_equals_the_counter_loop(factors, edge, zeros):
    for name, vol in VOLUMES:
        got = ref.downsample(vol, factors, edge, zeros)
        assert got.dtype == vol.dtype and got.shape == ref.level_shape(vol.shape, factors, edge)
        np.testing.assert_array_equal(got, loop_level(vol, factors, edge, zeros), err_msg=name)


def _one(values, zeros, dtype=np.uint64):
    vol = np.array(values, dtype=dtype).reshape(2, 2, 2)
    return int(ref.downsample(vol, (2, 2, 2), "crop", zeros)[0, 0, 0])


def test_tie_rules_by_hand():
    # "count": 0 is a value like any other, and of equally frequent values the smallest wins
    assert _one([5, 5, 5, 5, 3, 3, 3, 3], "count") == 3
    assert _one([0, 0, 0, 0, 3, 3, 3, 3], "count") == 0
    assert _one([9, 9, 9, 4, 4, 4, 1, 2], "count") == 4
    assert _one([2 ** 63, 2 ** 63, 1, 1, 7, 8, 9, 10], "count") == 1
    assert _one([2 ** 32, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 1, 2 ** 33, 2 ** 33, 2 ** 64 - 1, 2 ** 64 - 1], "count") == 2 ** 32
    # "ignore": the zeros do not vote; of equally frequent non-zero values the smallest wins
    assert _one([0, 0, 0, 0, 3, 3, 3, 3], "ignore") == 3
    assert _one([0, 0, 0, 0, 0, 9, 4, 0], "ignore") == 4
    assert _one([0, 0, 0, 0, 0, 2 ** 64 - 1, 2 ** 63, 0], "ignore") == 2 ** 63
    assert _one([0, 0, 0, 0, 0, 9, 9, 4], "ignore") == 9
    assert _one([0] * 8, "ignore") == 0
    # frequency beats size: the larger value wins when it is more frequent
    assert _one([2 ** 32 + 1, 2 ** 32 + 1, 2 ** 32 + 1, 1, 1, 0, 0, 5], "count") == 2 ** 32 + 1
    assert _one([2 ** 32 - 1] * 3 + [7] * 2 + [0] * 3, "count", np.uint32) == 0
    assert _one([2 ** 32 - 1] * 3 + [7] * 2 + [0] * 3, "ignore", np.uint32) == 2 ** 32 - 1


def test_cut_windows_count_only_the_voxels_present():
    # (3, 1, 1) under "partial": the last window holds one voxel, and padding never votes
    vol = np.array([4, 4, 0], dtype=np.uint32).reshape(3, 1, 1)
    np.testing.assert_array_equal(ref.downsample(vol, (2, 1, 1), "partial", "count").reshape(-1), [4, 0])
    vol = np.array([4, 6, 9], dtype=np.uint32).reshape(1, 1, 3)
    np.testing.assert_array_equal(ref.downsample(vol, (1, 1, 2), "partial", "ignore").reshape(-1), [4, 9])
    np.testing.assert_array_equal(ref.downsample(vol, (1, 1, 2), "crop", "ignore").reshape(-1), [4])


def test_a_thin_line_survives_only_when_zeros_are_ignored():
    vol = np.zeros((8, 8, 8), dtype=np.uint64)
    vol[3, 5, :] = 2 ** 40 + 3                     # a neurite one voxel thin
    counted = ref.downsample(vol, (2, 2, 2), "crop", "count")
    ignored = ref.downsample(vol, (2, 2, 2), "crop", "ignore")
    assert not counted.any()
    want = np.zeros((4, 4, 4), dtype=np.uint64)
    want[1, 2, :] = 2 ** 40 + 3
    np.testing.assert_array_equal(ignored, want)
