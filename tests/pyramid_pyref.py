"""Numpy restatement of one pyramid level, the tests' reference.

``factors = (fz, fy, fx)``, each 1 or 2.  Level voxel (z, y, x) reduces the source voxels ``[z fz, min(nz, (z + 1) fz))
x ...``.  ``edge="crop"``: ``n // f`` voxels per axis, no window is cut; ``"partial"``: ``ceil(n / f)``, the last window
of an axis may be cut.  Windows come from padding and reshaping: the volume is cut (crop) or padded (partial) to whole
windows, reshaped to ``(Lz, fz, Ly, fy, Lx, fx)`` and brought to ``(Lz, Ly, Lx, fz fy fx)``, with a boolean array of the
same shape that says which entries are voxels of the volume."""
import numpy as np

METHODS = ("mode", "mean", "max")
EDGES = ("crop", "partial")


def level_shape(shape, factors, edge="crop"):
    assert edge in EDGES
    return tuple(n // f if edge == "crop" else -(-n // f) for n, f in zip(shape, factors))


def windows(vol, factors, edge="crop"):
    """``(values, present)``: ``(Lz, Ly, Lx, fz fy fx)`` int64 values and the bools that mark the voxels of the volume
    among them (all of them under "crop")."""
    vol = np.asarray(vol)
    assert vol.ndim == 3 and all(f in (1, 2) for f in factors)
    level = level_shape(vol.shape, factors, edge)
    whole = tuple(l * f for l, f in zip(level, factors))
    cut = vol[tuple(slice(0, min(n, w)) for n, w in zip(vol.shape, whole))].astype(np.int64)
    pad = [(0, w - n) for n, w in zip(cut.shape, whole)]
    values = np.pad(cut, pad, constant_values=0)
    present = np.pad(np.ones(cut.shape, dtype=bool), pad, constant_values=False)
    split = (level[0], factors[0], level[1], factors[1], level[2], factors[2])
    order = (0, 2, 4, 1, 3, 5)
    k = factors[0] * factors[1] * factors[2]
    return (values.reshape(split).transpose(order).reshape(level + (k,)),
            present.reshape(split).transpose(order).reshape(level + (k,)))


def reduce_windows(values, present, method):
    """The reduction of windows ``(..., k)`` of which ``present`` marks the entries that count; every window has one
    at least."""
    values, present = np.asarray(values, dtype=np.int64), np.asarray(present, dtype=bool)
    assert present.any(axis=-1).all()
    if method == "max":
        return np.where(present, values, -1).max(axis=-1).astype(np.uint16)
    if method == "mean":
        total = np.where(present, values, 0).sum(axis=-1)
        count = present.sum(axis=-1)
        return np.rint(total.astype(np.float64) / count.astype(np.float64)).astype(np.uint16)   # half to even
    assert method == "mode"
    # per voxel of a window the frequency of its value among the window's voxels; the winner is the largest
    # count * 65536 + (65535 - value): the most frequent, of those the smallest
    same = (values[..., :, None] == values[..., None, :]) & present[..., None, :]
    count = same.sum(axis=-1)
    key = np.where(present, count * 65536 + (65535 - values), -1)
    best = key.argmax(axis=-1)
    return np.take_along_axis(values, best[..., None], axis=-1)[..., 0].astype(np.uint16)


def downsample(vol, factors=(2, 2, 2), method="mode", edge="crop"):
    """One level of a 3-D uint16 volume."""
    assert method in METHODS
    values, present = windows(vol, factors, edge)
    return reduce_windows(values, present, method)


def box(level, origin, extent):
    return level[tuple(slice(o, o + e) for o, e in zip(origin, extent))]
