"""CPU restatements for the region reads of a chunk store, and the stores their tests read.

``gather_boxes_ref`` is ``exabm4d_gather_boxes_dev`` in numpy; ``touched_ref`` finds the chunks a box touches by
enumerating its voxels; ``slice_boxes`` is numpy slicing with padding.  ``build_stores`` writes the two fixture volumes
with chunk streams made on the host (the C restatement of the coder and the bounded formats' Python references), so
that what a read must return is known without the code under test.
"""
import os

import numpy as np

import block_bounded_pyref
import bounded_pyref
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume


def gather_boxes_ref(pool, srcs, box_srcs, starts, box, dtype=np.uint16, offset=0.0, fill=0):
    """out[n][z][y][x] = the voxel at starts[n] + (z, y, x) from the first source of box_srcs[n] that holds it
    (``srcs``: records with base, stride_y, stride_z, z0, y0, x0, ez, ey, ex; elements of ``pool``), else ``fill``;
    float32 output is ``float32(value) - float32(offset)``, the fill as given."""
    dt = np.dtype(dtype)
    pool = np.asarray(pool, dtype=np.uint16)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    out = np.full((len(starts),) + tuple(box), fill, dtype=dt)
    for n, st in enumerate(starts):
        for k in reversed([int(k) for k in box_srcs[n] if k >= 0]):       # later entries first: the first one wins
            s = srcs[k]
            org = np.array([s["z0"], s["y0"], s["x0"]], dtype=np.int64)
            ext = np.array([s["ez"], s["ey"], s["ex"]], dtype=np.int64)
            lo, hi = np.maximum(st, org), np.minimum(st + np.array(box), org + ext)
            if np.any(hi <= lo):
                continue
            z, y, x = (np.arange(lo[a], hi[a]) - org[a] for a in range(3))
            idx = int(s["base"]) + z[:, None, None] * int(s["stride_z"]) + y[None, :, None] * int(s["stride_y"]) + \
                x[None, None, :]
            v = pool[idx]
            if dt == np.float32:
                v = v.astype(np.float32) - np.float32(offset)
            out[(n,) + tuple(slice(lo[a] - st[a], hi[a] - st[a]) for a in range(3))] = v
    return out


def touched_ref(shape, chunk, start, box):
    """The chunks (iz, iy, ix) a box touches inside the array, raster order: its voxels' coordinates // chunk."""
    per_axis = []
    for a in range(3):
        c = np.arange(int(start[a]), int(start[a]) + int(box[a]))
        per_axis.append(np.unique(c[(c >= 0) & (c < shape[a])] // chunk[a]))
    return [(int(z), int(y), int(x)) for z in per_axis[0] for y in per_axis[1] for x in per_axis[2]]


def slice_boxes(vol, starts, box, fill=0, dtype=None):
    """numpy slicing with padding: (N, *box) of ``vol`` at ``starts``, ``fill`` outside the array."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    out = np.full((len(starts),) + tuple(box), fill, dtype=dtype or vol.dtype)
    for n, st in enumerate(starts):
        lo, hi = np.maximum(st, 0), np.minimum(st + np.array(box), np.array(vol.shape))
        if np.any(hi <= lo):
            continue
        out[(n,) + tuple(slice(lo[a] - st[a], hi[a] - st[a]) for a in range(3))] = \
            vol[tuple(slice(lo[a], hi[a]) for a in range(3))]
    return out


# ---- the stores ---------------------------------------------------------------------------------------------
SHAPE_A, CHUNK_A = (37, 21, 70), (16, 16, 32)
SHAPE_B, CHUNK_B = (20, 20, 136), (8, 8, 64)
MASK_A = (slice(10, 20), slice(5, 12), slice(8, 24))


def volume(shape, split, seed=11):
    """Smooth (compressible) where x < split, uniform noise beyond: both modes of the bounded formats occur."""
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    rng = np.random.default_rng(seed)
    smooth = 200 + 3 * z + 2 * y + x + rng.normal(0, 6, shape)
    vol = np.where(x >= split, rng.integers(0, 65536, shape), smooth)
    return np.clip(vol, 0, 65535).astype(np.uint16)


def _container(blobs, shape, chunk):
    sizes = np.array([len(b) for b in blobs], dtype=np.uint32)
    offsets = np.zeros(len(blobs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes.astype(np.uint64) + 15) // 16 * 16)
    data = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for b, o in zip(blobs, offsets[:-1]):
        data[int(o):int(o) + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return EncodedVolume(data, offsets, sizes, shape, chunk, 2)


def build_stores(root, which="AB"):
    """-> {name: (path, expected (z, y, x) array, chunk streams)} for "A-exac2", "A-exac1", "A-dctq", "A-block",
    "B-exac2" and "B-dctq", written under ``root``."""
    from oracle import codec_oracle as co
    stores = {}

    def put(name, blobs, shape, chunk, expected, **kw):
        path = os.path.join(str(root), name)
        chunk_store.write_encoded(_container(blobs, shape, chunk), path, **kw)
        stores[name] = (path, expected, blobs)

    for tag, shape, chunk, split in (("A", SHAPE_A, CHUNK_A, 32), ("B", SHAPE_B, CHUNK_B, 64)):
        if tag not in which:
            continue
        vol = volume(shape, split)
        put(tag + "-exac2", [bytes(co.encode(c)) for c in co.chunks(vol, chunk)], shape, chunk, vol)
        blobs, rec, _ = bounded_pyref.encode_volume(vol, chunk, 4)
        put(tag + "-dctq", blobs, shape, chunk, rec, codec=BoundedDctCodec(4))
        if tag == "A":
            put("A-exac1", [bytes(co.encode(c, version=1)) for c in co.chunks(vol, chunk)], shape, chunk, vol,
                version=1)
            mask = np.zeros(shape, dtype=bool)
            mask[MASK_A] = True
            blobs, rec, _ = block_bounded_pyref.encode_volume(vol, chunk, 6, 0, mask)
            put("A-block", blobs, shape, chunk, rec, codec=BlockBoundedCodec(6, 0))
    return stores
