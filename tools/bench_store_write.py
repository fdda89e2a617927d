"""Writing patch batches into a chunk store, and denoising store to store.

usage: python tools/bench_store_write.py [--dir DIR] [--edge 512] [--patches 256] [--patch 64] [--reps 3]
                                         [--mode write | denoise | trace-run]
A seeded synthetic ``edge``^3 uint16 volume (``bench_store_read.synth``) is written once with ``ExacCodec(2)`` in 64^3
chunks (an existing store under DIR is reused).

``--mode write``: ``patches`` random ``patch``^3 boxes at unaligned starts inside it are written by
  (new) ``open_zarr(mode="r+").write_patches``, which re-codes the touched chunks only, and
  (old) the only route there was: ``read_zarr``, numpy assignment, ``write_zarr`` of the whole array,
each into its own copy of the store, warmed, then timed ``reps`` times with a host clock around work that ends in a
synchronisation, alternating inside one process; both stores must then read back equal.  One JSON line: medians,
``write_patches``' own phase seconds (``last_write``) and the scatter kernel's bytes.

``--mode denoise``: ``bm4d.denoise_store`` (``--chunk 256 --halo 8``) against ``read_zarr`` +
``denoise_chunked_streamed`` + ``write_zarr`` from the same tree, alternating, ``reps`` times after a warm-up; the two
destinations must hold the same files.  One JSON line: medians, ``denoise_store``'s phase seconds, and for both routes
the largest single device allocation and the most device memory held at a time, as far as they go through
``Context.alloc`` (the pipeline's scratch and the streamed form's device windows are the library's own and are not
seen).

``--mode trace-run`` only scatters the batch into the pool of the touched chunks a few times: the run to put under
``rocprofv3 --kernel-trace --stats``, whose time of ``scatter_boxes_kernel`` divides the scatter's bytes (source
voxels read + pool voxels written, from the shapes).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from aind_exaspim_image_compression import _native, bm4d  # noqa: E402
from aind_exaspim_image_compression.utils import chunk_store, store_write  # noqa: E402
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec  # noqa: E402
from bench_store_read import CHUNK, HBM_PEAK, synth  # noqa: E402


class AllocWatch:
    """Largest single ``Context.alloc`` and most bytes held at a time, between ``reset()`` and now."""

    def __init__(self):
        self.live = self.peak = self.largest = 0
        init, free = _native.DeviceBuffer.__init__, _native.DeviceBuffer.free
        watch = self

        def new_init(buf, ctx, nbytes):
            init(buf, ctx, nbytes)
            watch.live += buf.nbytes
            watch.peak, watch.largest = max(watch.peak, watch.live), max(watch.largest, buf.nbytes)

        def new_free(buf):
            if buf.ptr:
                watch.live -= buf.nbytes
            free(buf)

        _native.DeviceBuffer.__init__, _native.DeviceBuffer.free = new_init, new_free

    def reset(self):
        self.peak, self.largest = self.live, 0


def files_of(path):
    out = {}
    for root, _, names in os.walk(path):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), path)] = f.read()
    return out


def alternate(ctx, paths, reps):
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            times[k].append(time.perf_counter() - t0)
    return times


def report(out, times):
    for k, ts in times.items():
        out[k + "_ms"] = round(1e3 * float(np.median(ts)), 3)
        out[k + "_range_ms"] = [round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--halo", type=int, default=8)
    ap.add_argument("--mode", choices=("write", "denoise", "trace-run"), default="write")
    a = ap.parse_args()
    root = a.dir or tempfile.mkdtemp(prefix="store_write_")
    watch = AllocWatch()
    ctx = _native.context()
    base = os.path.join(root, "exac")
    chunks = (1, 1, CHUNK, CHUNK, CHUNK)
    if not os.path.exists(os.path.join(base, "zarr.json")):
        chunk_store.write_zarr(synth(a.edge), base, chunks=chunks, codec=ExacCodec(2))
    shape = (a.edge,) * 3
    rng = np.random.default_rng(1)
    starts = rng.integers(0, a.edge - a.patch + 1, (a.patches, 3))
    box = (a.patch,) * 3

    if a.mode in ("write", "trace-run"):
        values = rng.integers(100, 140, (a.patches,) + box).astype(np.uint16)
        union = np.zeros(shape, dtype=bool)
        for s in starts:
            union[s[0]:s[0] + a.patch, s[1]:s[1] + a.patch, s[2]:s[2] + a.patch] = True
        scatter_bytes = 2 * 2 * int(union.sum())          # every written voxel: one uint16 read, one written
        del union

    if a.mode == "trace-run":
        (g,) = store_write.plan_write(shape, (CHUNK,) * 3, starts, box, False, max_pool_bytes=1 << 40)
        d_src, pool = ctx.to_device(values), ctx.alloc(2 * g.pool_elems).zero()
        records = store_write.box_records(starts, box)
        for _ in range(5):
            ctx.scatter_boxes(d_src, values.size, np.uint16, records, pool, g.pool_elems, np.uint16, g.dsts, g.dst_boxes)
        ctx.sync()
        d_src.free()
        pool.free()
        print(json.dumps({"trace_run": True, "scatter_bytes_per_call": scatter_bytes, "calls": 5,
                          "chunks": len(g.chunks), "per_dst": int(g.dst_boxes.shape[1])}))
        return

    if a.mode == "write":
        new, old = os.path.join(root, "write-new"), os.path.join(root, "write-old")
        for p in (new, old):
            shutil.rmtree(p, ignore_errors=True)
            shutil.copytree(base, p)
        arr = chunk_store.open_zarr(new, mode="r+")
        split = {}

        def write_patches():
            arr.write_patches(starts, values, is_center=False)
            split.update(arr.last_write)

        def whole_array():
            vol = chunk_store.read_zarr(old)[0, 0].copy()
            for s, v in zip(starts, values):
                vol[s[0]:s[0] + a.patch, s[1]:s[1] + a.patch, s[2]:s[2] + a.patch] = v
            chunk_store.write_zarr(vol, old, chunks=chunks, codec=ExacCodec(2))

        paths = {"write_patches": write_patches, "read_zarr_assign_write_zarr": whole_array}
        for fn in paths.values():                         # warm both, and compare what they leave
            fn()
        assert files_of(new) == files_of(old)
        times = alternate(ctx, paths, a.reps)
        report({"mode": "write", "edge": a.edge, "patches": a.patches, "patch": a.patch, "reps": a.reps,
                "chunks_written": split["chunks"], "chunks_decoded": split["decoded"], "of_chunks": (a.edge // CHUNK) ** 3,
                "chunk_bytes_written": split["chunk_bytes"], "encode_calls": split["encode_calls"],
                "groups": split["groups"],
                "write_patches_split_ms": {k: round(1e3 * v, 3) for k, v in split["seconds"].items()},
                "scatter_bytes": scatter_bytes, "hbm_peak_bytes_per_s": HBM_PEAK}, times)
        return

    new, old = os.path.join(root, "denoise-new"), os.path.join(root, "denoise-old")
    sigma, offset = 6.0, 100.0
    stats, mem = {}, {}

    def store_to_store():
        watch.reset()
        stats.clear()
        bm4d.denoise_store(base, new, sigma, offset, chunk=a.chunk, halo=a.halo, stats=stats)
        mem["denoise_store"] = (watch.largest, watch.peak)

    def through_the_host():
        watch.reset()
        vol = chunk_store.read_zarr(base)[0, 0]
        res = bm4d.denoise_chunked_streamed(vol, sigma, offset, chunk=a.chunk, halo=a.halo)
        chunk_store.write_zarr(res, old, chunks=chunks, codec=ExacCodec(2))
        mem["read_denoise_streamed_write"] = (watch.largest, watch.peak)

    paths = {"denoise_store": store_to_store, "read_denoise_streamed_write": through_the_host}
    for fn in paths.values():
        fn()
    assert files_of(new) == files_of(old)
    times = alternate(ctx, paths, a.reps)
    report({"mode": "denoise", "edge": a.edge, "chunk": a.chunk, "halo": a.halo, "reps": a.reps,
            "bricks": stats["bricks"], "windows": stats["windows"],
            "denoise_store_split_ms": {k: round(1e3 * v, 3) for k, v in stats["seconds"].items()},
            "largest_alloc_bytes": {k: v[0] for k, v in mem.items()},
            "most_held_bytes": {k: v[1] for k, v in mem.items()}}, times)


if __name__ == "__main__":
    main()
