"""Reading patch batches out of a chunk store, three ways.

usage: python tools/bench_store_read.py [--dir DIR] [--edge 512] [--patches 256] [--patch 64] [--reps 3]
                                        [--trace-run]
A seeded synthetic ``edge``^3 uint16 volume is written once with ``ExacCodec(2)`` and once with
``BlockBoundedCodec(8, 1)`` (64^3 chunks; an existing store under DIR is reused), and ``patches`` random ``patch``^3
boxes inside it are read by
  (a) ``open_zarr(...).read_patches``, to the host and to the device,
  (b) what the store offered before: per patch, ``read_chunk`` of every chunk it touches and a numpy stitch,
  (c) ``read_zarr`` of the whole array, then numpy slicing.
Every path is warmed, then timed ``reps`` times with a host clock around work that ends in a synchronisation, the
paths alternating inside one process; the median goes into one JSON line per codec, with the chunks decoded per
patch, ``read_patches``' own split (file reads, decodes, gather) and the gather kernel's bytes (pool voxels read +
output written, from the shapes).  The three paths must return the same arrays.

``--trace-run`` only reads the batch to the device a few times from the exac store: the run to put under
``rocprofv3 --kernel-trace --stats``, whose time of ``gather_boxes_kernel`` divides the gather's bytes.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))

from aind_exaspim_image_compression import _native  # noqa: E402
from aind_exaspim_image_compression.utils import chunk_store  # noqa: E402
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec  # noqa: E402
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec  # noqa: E402

CHUNK = 64
HBM_PEAK = 8.0e12           # bytes/s, spec; about 6.3e12 is what a float4 copy reaches on this part


def synth(edge, seed=0):
    """Background counts with smooth structure, sparse bright voxels and noise."""
    rng = np.random.default_rng(seed)
    g = np.arange(edge, dtype=np.float32)
    base = 120.0 + 20.0 * np.sin(g / 37.0)[:, None, None] + 15.0 * np.cos(g / 53.0)[None, :, None] + \
        10.0 * np.sin(g / 29.0)[None, None, :]
    vol = base + rng.standard_normal((edge, edge, edge), dtype=np.float32) * 6.0
    bright = rng.random((edge, edge, edge), dtype=np.float32) < 0.01
    vol[bright] += 800.0 * rng.random(int(bright.sum()), dtype=np.float32)
    return np.clip(np.rint(vol), 0, 65535).astype(np.uint16)


def touched(start, patch):
    """The chunks a box inside the array touches."""
    return [(z, y, x) for z in range(start[0] // CHUNK, (start[0] + patch - 1) // CHUNK + 1)
            for y in range(start[1] // CHUNK, (start[1] + patch - 1) // CHUNK + 1)
            for x in range(start[2] // CHUNK, (start[2] + patch - 1) // CHUNK + 1)]


def stitch(path, starts, patch):
    """Path (b): one ``read_chunk`` per touched chunk of every patch."""
    out = np.empty((len(starts), patch, patch, patch), dtype=np.uint16)
    for n, st in enumerate(starts):
        for idx in touched(st, patch):
            c = chunk_store.read_chunk(path, *idx)
            org = [i * CHUNK for i in idx]
            lo = [max(s, o) for s, o in zip(st, org)]
            hi = [min(s + patch, o + e) for s, o, e in zip(st, org, c.shape)]
            out[(n,) + tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, st))] = \
                c[tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, org))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    root = a.dir or tempfile.mkdtemp(prefix="store_read_")
    ctx = _native.context()
    codecs = {"exac": ExacCodec(2), "exac-dctq-block": BlockBoundedCodec(8, 1)}
    vol = None
    for name, codec in codecs.items():
        path = os.path.join(root, name)
        if not os.path.exists(os.path.join(path, "zarr.json")) and not (a.trace_run and name != "exac"):
            vol = synth(a.edge) if vol is None else vol
            chunk_store.write_zarr(vol, path, chunks=(1, 1, CHUNK, CHUNK, CHUNK), codec=codec)
    rng = np.random.default_rng(1)
    starts = rng.integers(0, a.edge - a.patch + 1, (a.patches, 3))
    box = (a.patch,) * 3
    gather_bytes = 2 * 2 * a.patches * a.patch ** 3          # every box lies inside: read = written = 2 bytes a voxel

    if a.trace_run:
        arr = chunk_store.open_zarr(os.path.join(root, "exac"))
        for _ in range(5):
            arr.read_patches(starts, box, is_center=False, out="device").free()
        print(json.dumps({"trace_run": True, "gather_bytes_per_call": gather_bytes, "calls": 5}))
        return

    for name in codecs:
        path = os.path.join(root, name)
        arr = chunk_store.open_zarr(path)
        split = {}

        def a_host():
            r = arr.read_patches(starts, box, is_center=False)
            split.update(arr.last_read["seconds"])
            return r

        def a_device():
            d = arr.read_patches(starts, box, is_center=False, out="device")
            d.free()

        def b_chunks():
            return stitch(path, starts.tolist(), a.patch)

        def c_whole():
            whole = chunk_store.read_zarr(path)[0, 0]
            return np.stack([whole[s[0]:s[0] + a.patch, s[1]:s[1] + a.patch, s[2]:s[2] + a.patch] for s in starts])

        paths = {"read_patches_host": a_host, "read_patches_device": a_device, "read_chunk_stitch": b_chunks,
                 "read_zarr_slice": c_whole}
        want = a_host()                                      # warm every path, and compare what they return
        assert np.array_equal(b_chunks(), want) and np.array_equal(c_whole(), want)
        a_device()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():                      # alternating
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                times[k].append(time.perf_counter() - t0)
        out = {"codec": name, "edge": a.edge, "patches": a.patches, "patch": a.patch, "reps": a.reps,
               "chunks_decoded_per_patch_read_patches": round(arr.last_read["chunks"] / a.patches, 3),
               "chunks_decoded_per_patch_read_chunk":
                   round(sum(len(touched(s, a.patch)) for s in starts.tolist()) / a.patches, 3),
               "decode_calls": arr.last_read["decode_calls"], "groups": arr.last_read["groups"],
               "chunk_bytes_read": arr.last_read["chunk_bytes"],
               "read_patches_split_ms": {k: round(1e3 * v, 3) for k, v in split.items()},
               "gather_bytes": gather_bytes, "hbm_peak_bytes_per_s": HBM_PEAK}
        for k, ts in times.items():
            med = float(np.median(ts))
            out[k + "_ms"] = round(1e3 * med, 3)
            out[k + "_range_ms"] = [round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]
            out[k + "_patches_per_s"] = round(a.patches / med, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
