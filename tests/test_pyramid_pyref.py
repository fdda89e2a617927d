"""The numpy rule of a pyramid level (``pyramid_pyref``) on hand-written windows: the mode's tie rule,
the mean's exact halves, windows cut to 1, 2 and 4 voxels.  No GPU."""
import numpy as np
import pytest

import pyramid_pyref as ref

U16 = np.uint16


def _one(window, method, present=None):
    window = np.asarray(window, dtype=np.int64)
    present = np.ones(window.shape, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    return int(ref.reduce_windows(window[None], present[None], method)[0])


MODE_WINDOWS = {
    "all eight equal": ([7] * 8, 7),
    "all distinct: the mode is the minimum": ([9, 3, 8, 4, 7, 5, 6, 10], 3),
    "4 + 4": ([12, 5, 12, 5, 5, 12, 12, 5], 5),
    "2 + 2 + 2 + 2": ([40, 10, 30, 20, 10, 20, 30, 40], 10),
    "3 + 3 + 2, the pair is the minimum": ([9, 4, 6, 9, 6, 4, 6, 9], 6),
    "3 + 3 + 2, the pair is the maximum": ([2, 8, 5, 2, 5, 8, 5, 2], 2),
    "3 + 3 + 1 + 1: the smaller triple is neither min nor max": ([1, 6, 9, 6, 9, 6, 9, 50], 6),
    "a unique mode that is the maximum": ([1, 2, 3, 4, 5, 900, 900, 900], 900),
    "65535 and 0 present, 65535 wins": ([65535, 0, 65535, 1, 65535, 2, 0, 65535], 65535),
    "65535 and 0 tie": ([65535, 0, 65535, 0, 65535, 0, 0, 65535], 0),
}


@pytest.mark.parametrize("name", list(MODE_WINDOWS))
def test_mode_of_a_window(name):
    window, want = MODE_WINDOWS[name]
    assert _one(window, "mode") == want
    rng = np.random.default_rng(len(name))
    for _ in range(8):                                    # the order of the voxels does not matter
        assert _one(rng.permutation(window), "mode") == want
    assert _one(window, "max") == max(window)


def test_mean_rounds_exact_halves_to_even_both_ways():
    for window, want in [([0, 0, 0, 0, 0, 0, 0, 4], 0),               # 0.5 -> 0
                         ([0, 0, 0, 0, 0, 0, 0, 12], 2),              # 1.5 -> 2
                         ([0, 0, 0, 0, 0, 0, 0, 20], 2),              # 2.5 -> 2
                         ([65535] * 7 + [65531], 65534),              # 65534.5 -> 65534
                         ([65535] * 7 + [65523], 65534),              # 65533.5 -> 65534
                         ([0, 0, 0, 0, 0, 0, 0, 5], 1), ([0, 0, 0, 0, 0, 0, 0, 3], 0),
                         ([65535] * 8, 65535), ([1, 2, 3, 4, 5, 6, 7, 8], 4)]:            # 4.5 -> 4
        assert _one(window, "mean") == want, window
    for window, want in [([1, 2], 2), ([2, 3], 2), ([0, 1], 0), ([65534, 65535], 65534), ([1, 1, 1, 3], 2), ([1, 1, 1, 7], 2)]:
        present = [True] * len(window) + [False] * (8 - len(window))
        assert _one(window + [60000] * (8 - len(window)), "mean", present) == want, window


def test_partial_windows_of_1_2_and_4_voxels():
    filler = 65535                                        # what is not present never counts, whatever it holds
    for window, mode, mean, most in [([9], 9, 9, 9), ([0], 0, 0, 0), ([8, 3], 3, 6, 8), ([3, 3], 3, 3, 3),
                                     ([5, 2, 5, 2], 2, 4, 5), ([5, 2, 5, 9], 5, 5, 9), ([4, 3, 2, 1], 1, 2, 4)]:
        values = window + [filler] * (8 - len(window))
        present = [True] * len(window) + [False] * (8 - len(window))
        for order in (slice(None), slice(None, None, -1)):
            v, p = values[order], present[order]
            assert (_one(v, "mode", p), _one(v, "mean", p), _one(v, "max", p)) == (mode, mean, most), window


@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("factors", [(2, 2, 2), (1, 2, 2), (2, 2, 1), (2, 1, 1), (1, 1, 2)])
def test_downsample_against_a_loop(factors, edge):
    rng = np.random.default_rng(sum(factors))
    vol = rng.integers(0, 4, (5, 4, 7)).astype(U16)
    vol[-1, -1, -1] = 65535
    level = ref.level_shape(vol.shape, factors, edge)
    assert level == tuple((n // f) if edge == "crop" else (n + f - 1) // f for n, f in zip(vol.shape, factors))
    got = {m: ref.downsample(vol, factors, m, edge) for m in ref.METHODS}
    for m in ref.METHODS:
        assert got[m].shape == level and got[m].dtype == U16
    for z in range(level[0]):
        for y in range(level[1]):
            for x in range(level[2]):
                w = vol[z * factors[0]:(z + 1) * factors[0], y * factors[1]:(y + 1) * factors[1],
                        x * factors[2]:(x + 1) * factors[2]].reshape(-1).astype(np.int64)
                assert w.size in (1, 2, 4, 8) and (edge == "partial" or w.size == int(np.prod(factors)))
                counts = np.bincount(w)
                assert got["mode"][z, y, x] == int(np.flatnonzero(counts == counts.max())[0])
                assert got["max"][z, y, x] == w.max()
                q, r = divmod(int(w.sum()), w.size)
                assert got["mean"][z, y, x] == q + (1 if 2 * r > w.size or (2 * r == w.size and q % 2) else 0)


def test_a_mask_keeps_its_value_under_max():
    mask = np.zeros((4, 6, 6), dtype=U16)
    mask[1, 2, 3] = 40000
    level = ref.downsample(mask, (2, 2, 2), "max")
    assert level[0, 1, 1] == 40000 and int((level != 0).sum()) == 1
    assert not ref.downsample(mask, (2, 2, 2), "mode").any()
