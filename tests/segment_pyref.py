"""numpy restatement of the out-of-core component labelling (``utils/store_segment.py``,
``csrc/segment_kernels.hip``), worded from the header: windows, provisional labels, the three record kinds, the merge
and the relabelled bricks.  The window labeller is ``scipy.ndimage.label`` canonicalised to first-voxel labels (the
repository's own ``components_pyref.labels`` where scipy is missing); the merge is the package's ``merge_records``,
which is host code, or ``merge_by_loops`` below, a union-find with a Python loop per record that checks it."""
import itertools

import numpy as np

import components_pyref

try:
    from scipy import ndimage
except ImportError:                                      # pragma: no cover
    ndimage = None


def first_voxel_labels(seeds, connectivity):
    """uint64 labels of a boolean array: 1 + the linear index of the component's first voxel in raster order."""
    seeds = np.asarray(seeds, dtype=bool)
    if ndimage is None:
        return components_pyref.labels(seeds, connectivity).astype(np.uint64)
    structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    lab, n = ndimage.label(seeds, structure=structure)
    flat = lab.reshape(-1)
    # scipy numbers the components in raster order of their first voxels: the first occurrence of each number
    first = np.zeros(n + 1, dtype=np.uint64)
    idx = np.flatnonzero(flat)
    num, at = np.unique(flat[idx], return_index=True)
    first[num] = idx[at].astype(np.uint64) + np.uint64(1)
    return first[flat].reshape(seeds.shape)


def whole_volume(seeds, connectivity, min_voxels=0, relabel=False):
    """(labels uint64, final labels of the kept components, their sizes): the expectation of the whole scheme."""
    lab = first_voxel_labels(seeds, connectivity)
    ids, counts = np.unique(lab[lab != 0], return_counts=True)
    keep = counts >= max(0, int(min_voxels))
    becomes = np.where(keep, ids, 0).astype(np.uint64)
    if relabel:
        becomes = np.where(keep, np.cumsum(keep), 0).astype(np.uint64)
    table = np.zeros(lab.size + 1, dtype=np.uint64)
    table[ids.astype(np.int64)] = becomes
    return table[lab.astype(np.int64)], becomes[keep], counts[keep].astype(np.uint64)


def bricks_of(shape, brick):
    """(origin, extent, window extent) of the bricks of shape ``brick`` that partition ``shape``, in raster order; a
    window is the brick and one voxel more on the high side of each axis, cut at the faces."""
    axes = [[(o, min(b, n - o)) for o in range(0, n, b)] for n, b in zip(shape, brick)]
    out = []
    for r in itertools.product(*axes):
        origin, extent = tuple(q[0] for q in r), tuple(q[1] for q in r)
        window = tuple(min(n, o + e + 1) - o for o, e, n in zip(origin, extent, shape))
        out.append((origin, extent, window))
    return out


def window_labels(seeds, origin, window, connectivity):
    """The window's own labels (1 + WINDOW index of the first voxel): what ``component_seeds_u16`` makes of it."""
    sl = tuple(slice(o, o + w) for o, w in zip(origin, window))
    return first_voxel_labels(seeds[sl], connectivity)


def provisional(lab, shape, origin, window):
    """Window labels -> provisional labels: 1 + the VOLUME index of the voxel at window index label - 1."""
    idx = lab.astype(np.int64) - 1
    z, y, x = np.unravel_index(np.maximum(idx, 0), window)
    vol = ((z + origin[0]) * shape[1] + (y + origin[1])) * shape[2] + (x + origin[2]) + 1
    return np.where(lab != 0, vol, 0).astype(np.uint64)


def collect(seeds, origin, extent, window, connectivity):
    """(halo, face, size, provisional labels of the window) of one brick, records sorted."""
    shape = seeds.shape
    prov = provisional(window_labels(seeds, origin, window, connectivity), shape, origin, window)
    zz, yy, xx = np.meshgrid(*[np.arange(o, o + w) for o, w in zip(origin, window)], indexing="ij")
    vox = ((zz * shape[1] + yy) * shape[2] + xx).astype(np.uint64)
    inside = (zz < origin[0] + extent[0]) & (yy < origin[1] + extent[1]) & (xx < origin[2] + extent[2])
    low = ((zz == origin[0]) & (origin[0] > 0)) | ((yy == origin[1]) & (origin[1] > 0)) | \
          ((xx == origin[2]) & (origin[2] > 0))
    seed = prov != 0
    halo = np.stack([vox[seed & ~inside], prov[seed & ~inside]], axis=1)
    face = np.stack([vox[seed & inside & low], prov[seed & inside & low]], axis=1)
    ids, own = np.unique(prov[seed & inside], return_counts=True)
    size = np.stack([ids, own.astype(np.uint64)], axis=1)
    return _sorted(halo), _sorted(face), _sorted(size), prov


def _sorted(rec):
    rec = np.asarray(rec, dtype=np.uint64).reshape(-1, 2)
    return rec[np.lexsort((rec[:, 1], rec[:, 0]))]


def merge_by_loops(halo, face, size):
    """``merge_records`` by a plain union-find: (keys, vals, table)."""
    halo, face, size = (np.asarray(r, dtype=np.uint64).reshape(-1, 2) for r in (halo, face, size))
    parent = {int(l): int(l) for l in np.concatenate([size[:, 0], halo[:, 1], face[:, 1]])}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    owner = {}
    for v, l in face:
        owner.setdefault(int(v), int(l))
    for v, l in halo:
        if int(v) not in owner:
            raise RuntimeError("a halo voxel without a face record")
        a, b = find(int(l)), find(owner[int(v)])
        if a != b:
            parent[max(a, b)] = min(a, b)
    keys = np.array(sorted(parent), dtype=np.uint64)
    vals = np.array([find(int(k)) for k in keys], dtype=np.uint64)
    sums = {}
    for l, c in size:
        r = find(int(l))
        sums[r] = sums.get(r, 0) + int(c)
    table = np.array(sorted(sums.items()), dtype=np.uint64).reshape(-1, 2)
    return keys, vals, table


def components(seeds, brick, connectivity, min_voxels=0, relabel=False, merge=None):
    """The whole scheme on a boolean volume in bricks of shape ``brick``: (labels uint64, kept labels, sizes)."""
    from aind_exaspim_image_compression.utils import store_segment
    merge = merge or store_segment.merge_records
    seeds = np.asarray(seeds, dtype=bool)
    plan = bricks_of(seeds.shape, brick)
    parts = [collect(seeds, o, e, w, connectivity) for o, e, w in plan]
    cat = [np.concatenate([p[i] for p in parts]) for i in range(3)]
    keys, vals, table = merge(*cat)
    becomes = store_segment.final_labels(table, min_voxels, relabel)
    out_vals = becomes[np.searchsorted(table[:, 0], vals)] if vals.size else vals
    out = np.zeros(seeds.shape, dtype=np.uint64)
    for (origin, extent, window), part in zip(plan, parts):
        prov = part[3][:extent[0], :extent[1], :extent[2]]
        final = np.where(prov != 0, out_vals[np.minimum(np.searchsorted(keys, prov), max(keys.size - 1, 0))]
                         if keys.size else prov, 0)
        out[tuple(slice(o, o + e) for o, e in zip(origin, extent))] = final
    kept = becomes != 0
    return out, becomes[kept], table[kept, 1]
