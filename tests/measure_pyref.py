"""Plain numpy restatement of measuring a box: the counts and the wide noise table of a volume, and of
a box of it under the rule that a cell belongs to the box that holds its origin.  Cells, ``s``, ``|d|`` and the level
come from ``noise_pyref``; the wide bin is found octave by octave, and a wide bin's lowest value by looking it up among
all ``m``, neither the way the package computes them."""
import numpy as np

import noise_pyref as npr

LEVELS = npr.LEVELS
BINS = npr.BINS
WIDE_BINS = 16384
COUNT_BINS = 65536
M_MAX = 4 * 65535


def wide_bin(m):
    m = np.asarray(m, dtype=np.int64)
    w = np.where(m < BINS, m, -1)
    for j in range(1, 7):
        octave = (m >= (2048 << j)) & (m < (4096 << j))
        w = np.where(octave, BINS + (j - 1) * 2048 + (m >> j) - 2048, w)
    assert m.size == 0 or w.min() >= 0
    return w


def wide_low_values():
    """v0[w] for every wide bin: the first m that falls into it."""
    w = wide_bin(np.arange(M_MAX + 1))
    bins, first = np.unique(w, return_index=True)
    assert np.array_equal(bins, np.arange(WIDE_BINS))
    return first.astype(np.int64)


def fold(wide, shift):
    """The table at ``shift`` from a wide table, bin by bin."""
    v0 = wide_low_values()
    hist = np.zeros((LEVELS, BINS), dtype=np.uint64)
    for w in np.nonzero(wide.sum(axis=0))[0].tolist():
        hist[:, min(v0[w] >> shift, BINS - 1)] += wide[:, w].astype(np.uint64)
    return hist


def _box_slices(b0, bd):
    return tuple(slice(o, o + e) for o, e in zip(b0, bd))


def _counts(values):
    return np.bincount(values.reshape(-1).astype(np.int64), minlength=COUNT_BINS).astype(np.uint64)


def box_tables(vol, b0=None, bd=None, mask=None):
    """``(counts, wide, sum_s)`` of the box ``b0 + [0, bd)`` of a uint16 volume (the whole volume by default): its
    voxels, and the cells of the volume's even grid whose origins lie in it.  With a ``mask`` each is a pair
    ``[foreground, background]`` (leading axis 2): a voxel where its mask says, a cell in the background only if all
    eight of its voxels are."""
    vol = np.asarray(vol)
    assert vol.dtype == np.uint16 and vol.ndim == 3
    b0 = (0, 0, 0) if b0 is None else tuple(b0)
    bd = vol.shape if bd is None else tuple(bd)
    box = vol[_box_slices(b0, bd)]
    cells = tuple(n // 2 for n in vol.shape)
    wide = np.zeros((2, LEVELS, WIDE_BINS), dtype=np.int64)
    sum_s = np.zeros((2, LEVELS), dtype=np.int64)
    if min(cells) > 0:
        s, m, _ = npr.cell_values(vol)
        origin = np.meshgrid(*[2 * np.arange(c) for c in cells], indexing="ij")
        owned = np.ones(cells, dtype=bool)
        for a in range(3):
            owned &= (origin[a] >= b0[a]) & (origin[a] < b0[a] + bd[a])
        if mask is None:
            table = np.zeros(cells, dtype=np.int64)
        else:
            any_fg = np.zeros(cells, dtype=bool)
            mk = np.asarray(mask)[:2 * cells[0], :2 * cells[1], :2 * cells[2]] != 0
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        any_fg |= mk[dz::2, dy::2, dx::2]
            table = np.where(any_fg, 0, 1)
        owned, table = owned.reshape(-1), table.reshape(-1)
        s, m, table = s[owned], m[owned], table[owned]
        lv = npr.level_of(s)
        np.add.at(wide, (table, lv, wide_bin(m)), 1)
        np.add.at(sum_s, (table, lv), s)
    wide, sum_s = wide.astype(np.uint64), sum_s.astype(np.uint64)
    if mask is None:
        return _counts(box), wide[0], sum_s[0]
    mbox = np.asarray(mask)[_box_slices(b0, bd)] != 0
    return np.stack([_counts(box[mbox]), _counts(box[~mbox])]), wide, sum_s


def partition(shape, cuts):
    """The boxes ``(b0, bd)`` of cutting ``shape`` at ``cuts`` = three lists of inner cut positions."""
    edges = [[0] + list(c) + [n] for c, n in zip(cuts, shape)]
    return [((z0, y0, x0), (z1 - z0, y1 - y0, x1 - x0))
            for z0, z1 in zip(edges[0], edges[0][1:])
            for y0, y1 in zip(edges[1], edges[1][1:])
            for x0, x1 in zip(edges[2], edges[2][1:])]


def octave_volume(shape=(22, 19, 27), seed=5):
    """Noise at 300 +- 20, a slab of checkerboards whose amplitude runs through 2^8 .. 2^16 along x so that |d| falls
    into every octave of the wide table, and one cell of 0 / 65535 that gives |d| = 4 * 65535."""
    rng = np.random.default_rng(seed)
    v = rng.normal(300.0, 20.0, shape)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    checker = (z + y + x) & 1
    amplitude = 2.0 ** (8 + (x // 2) % 9)
    slab = (z >= 4) & (z < 14)
    v = np.where(slab, v + checker * amplitude, v)
    vol = np.rint(np.clip(v, 0, 65535)).astype(np.uint16)
    vol[0:2, 0:2, 0:2] = (checker[0:2, 0:2, 0:2] * 65535).astype(np.uint16)
    return vol
