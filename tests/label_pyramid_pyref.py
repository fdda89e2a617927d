"""Numpy restatement of one pyramid level of a label volume, the tests' reference.

The geometry is ``pyramid_pyref``'s.  The values are uint32 / uint64 ids that compare as unsigned integers and never
leave their dtype (no int64, no float: 2^63 and 2^64 - 1 must survive).  Per window the values are sorted with the
entries that are no voxels of the volume moved behind them, the runs of equal values are measured, and the longest run
wins, of runs of one length the first, which is the smallest value.  ``zeros="ignore"``: the zeros are moved behind as
well, so the winner is the most frequent non-zero value; a window without one gives 0."""
import numpy as np

EDGES = ("crop", "partial")
ZEROS = ("count", "ignore")


def level_shape(shape, factors, edge="crop"):
    assert edge in EDGES
    return tuple(n // f if edge == "crop" else -(-n // f) for n, f in zip(shape, factors))


def windows(vol, factors, edge="crop"):
    """``(values, present)``: ``(Lz, Ly, Lx, fz fy fx)`` values of the volume's dtype and the bools that mark the voxels
    of the volume among them (all of them under "crop")."""
    vol = np.asarray(vol)
    assert vol.dtype in (np.dtype(np.uint32), np.dtype(np.uint64))
    assert vol.ndim == 3 and all(f in (1, 2) for f in factors)
    level = level_shape(vol.shape, factors, edge)
    whole = tuple(l * f for l, f in zip(level, factors))
    cut = vol[tuple(slice(0, min(n, w)) for n, w in zip(vol.shape, whole))]
    pad = [(0, w - n) for n, w in zip(cut.shape, whole)]
    values = np.pad(cut, pad, constant_values=0)
    present = np.pad(np.ones(cut.shape, dtype=bool), pad, constant_values=False)
    split = (level[0], factors[0], level[1], factors[1], level[2], factors[2])
    order = (0, 2, 4, 1, 3, 5)
    k = factors[0] * factors[1] * factors[2]
    assert values.dtype == vol.dtype
    return (values.reshape(split).transpose(order).reshape(level + (k,)),
            present.reshape(split).transpose(order).reshape(level + (k,)))


def reduce_windows(values, present, zeros="count"):
    """The mode of windows ``(..., k)`` of which ``present`` marks the entries that count; every window has one at
    least."""
    assert zeros in ZEROS
    values, present = np.asarray(values), np.asarray(present, dtype=bool)
    dtype = values.dtype
    assert dtype in (np.dtype(np.uint32), np.dtype(np.uint64)) and present.any(axis=-1).all()
    counted = present & (values != 0) if zeros == "ignore" else present
    k = values.shape[-1]
    # the counted entries first, in ascending (unsigned) order: sort by (not counted, value)
    order = np.lexsort((values, ~counted), axis=-1)
    v = np.take_along_axis(values, order, axis=-1)
    c = np.take_along_axis(counted, order, axis=-1)
    # run[..., i]: the length of the run of equal counted values that ends at i
    run = np.zeros(v.shape, dtype=np.int64)
    run[..., 0] = c[..., 0]
    for i in range(1, k):
        same = c[..., i] & (v[..., i] == v[..., i - 1])
        run[..., i] = np.where(c[..., i], np.where(same, run[..., i - 1] + 1, 1), 0)
    longest = run.max(axis=-1, keepdims=True)
    # the first entry at which a run reaches the greatest length: the smallest such value
    first = np.argmax(run == longest, axis=-1)
    best = np.take_along_axis(v, first[..., None], axis=-1)[..., 0]
    out = np.where(longest[..., 0] > 0, best, np.zeros((), dtype=dtype))
    assert out.dtype == dtype
    return out


def downsample(vol, factors=(2, 2, 2), edge="crop", zeros="count"):
    """One level of a 3-D uint32 / uint64 volume."""
    values, present = windows(vol, factors, edge)
    return reduce_windows(values, present, zeros)


def box(level, origin, extent):
    return level[tuple(slice(o, o + e) for o, e in zip(origin, extent))]
