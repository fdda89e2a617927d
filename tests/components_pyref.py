"""numpy-only restatement of the connected-component entries (include/exabm4d.h): canonical labels by
iterated minimum propagation over the neighbourhood until nothing changes, sizes by ``bincount``, and the box-and-halo
form of ``exabm4d_component_seeds_u16_dev`` worded from the header.  scipy is not needed (and is only compared against
where it is importable, in the host tests)."""
import itertools

import numpy as np

from foreground_pyref import ball_dilate

BIG = np.iinfo(np.int64).max


def offsets(connectivity):
    """The neighbour offsets (dz, dy, dx): the 6 faces, or all 26 of the 3 x 3 x 3 cube."""
    if connectivity not in (6, 26):
        raise ValueError("connectivity is 6 or 26")
    every = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    return every if connectivity == 26 else [d for d in every if sum(map(abs, d)) == 1]


def _shifted(a, d, fill):
    """``out[p] = a[p + d]``, ``fill`` where p + d lies outside."""
    out = np.full_like(a, fill)
    src = tuple(slice(max(0, k), a.shape[i] + min(0, k)) for i, k in enumerate(d))
    dst = tuple(slice(max(0, -k), a.shape[i] + min(0, -k)) for i, k in enumerate(d))
    out[dst] = a[src]
    return out


def labels(seeds, connectivity):
    """Canonical labels (uint32) of the boolean (z, y, x) array ``seeds``: 1 + the linear index of the first voxel, in
    raster order, of the voxel's component; background 0.  Every seed starts with its own index + 1 and takes the
    minimum over its neighbourhood until nothing changes; between two rounds a seed may also take the label of the voxel
    its label names (a voxel of its own component), which only shortens long chains."""
    seeds = np.asarray(seeds, dtype=bool)
    lab = np.where(seeds, np.arange(1, seeds.size + 1, dtype=np.int64).reshape(seeds.shape), BIG)
    offs = offsets(connectivity)
    while True:
        new = lab
        for d in offs:
            new = np.where(seeds, np.minimum(new, _shifted(new, d, BIG)), BIG)     # (only seeds carry a label on)
        for _ in range(2):
            flat = new.reshape(-1)
            new = np.where(seeds, flat[np.where(seeds, new, 1) - 1].reshape(seeds.shape), BIG)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(seeds, lab, 0).astype(np.uint32)


def sizes(lab):
    """uint32, shaped like ``lab``: at linear index label - 1 the voxels of that component, else 0."""
    counts = np.bincount(lab.reshape(-1).astype(np.int64), minlength=lab.size + 1)[1:lab.size + 1]
    return counts.astype(np.uint32).reshape(lab.shape)


def kept(seeds, min_voxels, connectivity):
    """The seeds whose component has at least ``min_voxels`` voxels (bool): the whole-array filter."""
    lab = labels(seeds, connectivity)
    big = np.concatenate([[False], sizes(lab).reshape(-1) >= int(min_voxels)])
    return big[lab]


def count_components(lab):
    return int(np.count_nonzero(lab.reshape(-1) == np.arange(1, lab.size + 1)))


def relabel(lab):
    """Labels 1..n in raster order of the components' first voxels (``scipy.ndimage.label``'s numbering)."""
    flat = lab.reshape(-1).astype(np.int64)
    firsts = np.flatnonzero(flat == np.arange(1, flat.size + 1))
    table = np.zeros(flat.size + 1, dtype=np.int32)
    table[firsts + 1] = np.arange(1, firsts.size + 1)
    return table[flat].reshape(lab.shape), int(firsts.size)


def region(vol_shape, box_origin, box_dims, min_voxels):
    """(lo, hi) per axis of the labelled region: the box grown by ``min_voxels - 1`` and cut at the volume's faces."""
    g = max(0, int(min_voxels) - 1)
    lo = [max(0, o - g) for o in box_origin]
    hi = [min(n, o + d + g) for o, d, n in zip(box_origin, box_dims, vol_shape)]
    return lo, hi


def component_seeds(vol, cut, min_voxels, connectivity, box_origin, box_dims, count_origin=None, count_dims=None):
    """``exabm4d_component_seeds_u16_dev`` for the box of the VOLUME ``vol`` (what a window holds past the faces is
    never a seed, so the volume says it all): a voxel is a seed where ``vol >= cut`` inside the labelled region;
    labels and sizes are the region's own; a seed is kept where its component IN THE REGION has at least ``min_voxels``
    voxels.  Returns ``{"labels", "sizes"}`` (region-shaped uint32), ``"seeds_u16"`` (box-shaped, 1 / 0) and
    ``"counts"``: the seeds, the kept seeds and the dropped components whose first voxel lies in the count box (default
    the box)."""
    vol = np.asarray(vol)
    lo, hi = region(vol.shape, box_origin, box_dims, min_voxels)
    seeds = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.int64) >= int(cut)
    lab = labels(seeds, connectivity)
    siz = sizes(lab)
    keep = np.concatenate([[False], siz.reshape(-1) >= int(min_voxels)])[lab]
    first = lab.reshape(-1) == np.arange(1, lab.size + 1)
    dropped_first = (first & (siz.reshape(-1) < int(min_voxels))).reshape(lab.shape)
    inner = tuple(slice(o - l, o - l + d) for o, l, d in zip(box_origin, lo, box_dims))
    c0 = box_origin if count_origin is None else count_origin
    cd = box_dims if count_dims is None else count_dims
    cnt = tuple(slice(o - l, o - l + d) for o, l, d in zip(c0, lo, cd))
    counts = (int(seeds[cnt].sum()), int(keep[cnt].sum()), int(dropped_first[cnt].sum()))
    return {"labels": lab, "sizes": siz, "seeds_u16": keep[inner].astype(np.uint16), "counts": counts}


def filtered_mask(seeds, min_voxels, connectivity, dilate):
    """Threshold (done by the caller), filter, dilate: the whole-volume mask with ``min_voxels`` (0: no filter)."""
    seeds = np.asarray(seeds, dtype=bool)
    return ball_dilate(kept(seeds, min_voxels, connectivity) if min_voxels else seeds, dilate)
