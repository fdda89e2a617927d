"""CPU restatements for the region writes of a chunk store.

``scatter_boxes_ref`` is ``exabm4d_scatter_boxes_dev`` in numpy; ``assign_boxes`` is numpy's ``for n: arr[box n] =
v[n]`` with the parts outside the array dropped; ``plan_ref`` finds the touched chunks and their states by enumerating
voxels; ``counts_ref`` is the float32 -> uint16 conversion; ``host_blobs`` codes a volume's chunks with the host coders
the fixture stores of ``region_pyref`` were made with.
"""
import numpy as np

import block_bounded_pyref
import bounded_pyref
import region_pyref


def counts_ref(v, offset):
    """uint16(rint(clip(float32(v) + float32(offset), 0, 65535))), NaN -> 0."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(v, dtype=np.float32) + np.float32(offset)
        t = np.where(np.isnan(t), np.float32(0), t)
        return np.rint(np.clip(t, np.float32(0), np.float32(65535))).astype(np.uint16)


def scatter_boxes_ref(src, boxes, pool, dsts, dst_boxes, offset=0.0):
    """-> a copy of ``pool`` in which every voxel of every destination has the value of the last listed box that holds
    it (list entries applied first to last, so the last wins; -1 skipped); the rest is untouched.  ``src`` float32 and
    ``pool`` uint16: ``counts_ref``; otherwise the element types agree and values are copied."""
    src, out = np.asarray(src).reshape(-1), np.array(pool).reshape(-1).copy()
    convert = src.dtype == np.float32 and out.dtype == np.uint16
    assert convert or src.dtype == out.dtype
    for d, lst in zip(dsts, dst_boxes):
        d_org = np.array([d["z0"], d["y0"], d["x0"]], dtype=np.int64)
        d_ext = np.array([d["ez"], d["ey"], d["ex"]], dtype=np.int64)
        for k in (int(k) for k in lst if k >= 0):
            b = boxes[k]
            b_org = np.array([b["z0"], b["y0"], b["x0"]], dtype=np.int64)
            b_ext = np.array([b["ez"], b["ey"], b["ex"]], dtype=np.int64)
            lo, hi = np.maximum(d_org, b_org), np.minimum(d_org + d_ext, b_org + b_ext)
            if np.any(hi <= lo):
                continue

            def index(r, org):
                z, y, x = (np.arange(lo[a], hi[a]) - org[a] for a in range(3))
                return int(r["base"]) + z[:, None, None] * int(r["stride_z"]) + \
                    y[None, :, None] * int(r["stride_y"]) + x[None, None, :]
            v = src[index(b, b_org)]
            out[index(d, d_org)] = counts_ref(v, offset) if convert else v
    return out


def assign_boxes(vol, starts, values):
    """``for n: vol[box n] = values[n]`` on a copy, the parts of a box outside ``vol`` dropped."""
    out = vol.copy()
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    for st, v in zip(starts, values):
        lo, hi = np.maximum(st, 0), np.minimum(st + np.array(v.shape), np.array(vol.shape))
        if np.any(hi <= lo):
            continue
        out[tuple(slice(lo[a], hi[a]) for a in range(3))] = v[tuple(slice(lo[a] - st[a], hi[a] - st[a])
                                                                    for a in range(3))]
    return out


def plan_ref(shape, chunk, starts, boxes, exists=lambda *idx: True):
    """{(iz, iy, ix): state} of the chunks the boxes touch, by enumeration: a chunk is "covered" when one box alone
    holds every voxel of its extent, else "decode" when ``exists`` says it is stored, else "zero"."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 3)
    boxes = np.broadcast_to(np.asarray(boxes, dtype=np.int64), starts.shape)
    states = {}
    for st, box in zip(starts, boxes):
        for idx in region_pyref.touched_ref(shape, chunk, st, box):
            held = np.zeros(shape, dtype=bool)
            lo, hi = np.maximum(st, 0), np.minimum(st + box, np.array(shape))
            held[tuple(slice(lo[a], hi[a]) for a in range(3))] = True
            ext = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunk, shape))
            if held[ext].all():
                states[idx] = "covered"
            else:
                states.setdefault(idx, "decode" if exists(*idx) else "zero")
    return states


def host_blobs(vol, chunk, kind="exac2", mask=None):
    """{(iz, iy, ix): stream} of ``vol``'s chunks from the host coders: "exac2" / "exac1" (the C restatement),
    "dctq" (``bounded_pyref``, max_error 4) or "block" (``block_bounded_pyref``, bounds 6 / 0 with ``mask``)."""
    from oracle import codec_oracle as co
    if kind == "exac2":
        blobs = [bytes(co.encode(c)) for c in co.chunks(vol, chunk)]
    elif kind == "exac1":
        blobs = [bytes(co.encode(c, version=1)) for c in co.chunks(vol, chunk)]
    elif kind == "dctq":
        blobs = [bytes(b) for b in bounded_pyref.encode_volume(vol, chunk, 4)[0]]
    else:
        m = np.zeros(vol.shape, dtype=bool) if mask is None else mask
        blobs = [bytes(b) for b in block_bounded_pyref.encode_volume(vol, chunk, 6, 0, m)[0]]
    grid = [-(-s // c) for s, c in zip(vol.shape, chunk)]
    keys = [(z, y, x) for z in range(grid[0]) for y in range(grid[1]) for x in range(grid[2])]
    assert len(keys) == len(blobs)
    return dict(zip(keys, blobs))
