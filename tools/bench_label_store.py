"""The label codec and the label store on one MI355X.

usage: python tools/bench_label_store.py [--dir DIR] [--edge 512] [--patches 256] [--patch 64] [--reps 5] [--out FILE]

The volume is synthetic and seeded (``synth``): ``edge``^3 uint64 labels over a zero background -- tubes that wander
along z (radius 2..6) and balls (radius 6..24) with ids near 2^40, and one corner region of an eighth of the edge
filled with speckle (a random id out of 400 per voxel), so that every block class occurs.  It is written once as a raw
``.npy`` (what the parent commit's samplers read through ``np.memmap``) and once as an ``exac-labels`` store of 64^3
chunks.  Measured, each after warm-up, ``reps`` times, the median reported, with a host clock around work that ends
in a synchronisation of the stream:

* ``encode``: ``Context.label_encode`` of the device-resident volume into a device container (size pass, scans,
  write pass); ``decode``: ``Context.label_decode`` of that container into a device volume; ``copy``: a device copy
  of the decoded bytes (``torch``), the memory bound both are set against;
* stored bytes, next to byte shuffle + zstd level 5 of the same chunks through the machine's libzstd
  (``oracle/zstd_ref.py``), the family the reference's Blosc codec belongs to;
* ``patches`` random ``patch``^3 label patches: ``LabelArray.read_patches`` to the device and to the host, against
  the path the samplers had before -- ``np.memmap`` of the raw volume + ``read_label_patches`` + ``to_device`` -- with
  warm files for both, the two alternating; the patches must be equal.

One JSON line goes to stdout and, with ``--out``, to a file.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))

from aind_exaspim_image_compression import _native  # noqa: E402
from aind_exaspim_image_compression.machine_learning.sampling import read_label_patches  # noqa: E402
from aind_exaspim_image_compression.utils import chunk_store  # noqa: E402
from aind_exaspim_image_compression.utils.label_codec import LabelCodec  # noqa: E402

CHUNK = 64


def synth(edge, seed=0):
    """Tubes and balls with large ids over zeros, and a speckled corner; see the module docstring."""
    rng = np.random.default_rng(seed)
    vol = np.zeros((edge, edge, edge), dtype=np.uint64)
    big = np.uint64(1) << np.uint64(40)
    next_id = 1
    for _ in range(max(4, edge * edge // 1200)):                  # tubes along z
        r = rng.uniform(2.0, 6.0)
        cy, cx = rng.uniform(8, edge - 8, 2)
        py, px = rng.uniform(0, 6.28, 2)
        wy, wx = rng.uniform(20.0, 60.0, 2)
        z0 = int(rng.integers(0, edge // 2))
        z1 = int(rng.integers(z0 + edge // 4, edge + 1))
        label = big + np.uint64(7919 * next_id)
        next_id += 1
        for z in range(z0, min(z1, edge)):
            y, x = cy + 10.0 * np.sin(z / wy + py), cx + 10.0 * np.cos(z / wx + px)
            ya, yb = max(int(y - r - 1), 0), min(int(y + r + 2), edge)
            xa, xb = max(int(x - r - 1), 0), min(int(x + r + 2), edge)
            if ya >= yb or xa >= xb:
                continue
            yy, xx = np.ogrid[ya:yb, xa:xb]
            vol[z, ya:yb, xa:xb][(yy - y) ** 2 + (xx - x) ** 2 < r * r] = label
    for _ in range(max(2, edge // 8)):                            # balls
        r = rng.uniform(6.0, 24.0)
        c = rng.uniform(0, edge, 3)
        lo = [max(int(v - r - 1), 0) for v in c]
        hi = [min(int(v + r + 2), edge) for v in c]
        if any(a >= b for a, b in zip(lo, hi)):
            continue
        zz, yy, xx = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        inside = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 < r * r
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][inside] = big + np.uint64(7919 * next_id)
        next_id += 1
    s = max(edge // 8, 1)                                         # speckle
    vol[:s, :s, :s] = rng.integers(1, 401, (s, s, s)).astype(np.uint64)
    return vol


def median_seconds(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from oracle import zstd_ref

    work = args.dir or tempfile.mkdtemp(prefix="label_store_")
    os.makedirs(work, exist_ok=True)
    edge, shape, chunk = args.edge, (args.edge,) * 3, (CHUNK,) * 3
    vol = synth(edge)
    raw_path = os.path.join(work, "labels_raw.npy")
    np.save(raw_path, vol)
    ctx = _native.context(0)
    codec = LabelCodec(8)
    res = {"tool": "bench_label_store", "edge": edge, "dtype": "uint64", "chunk": CHUNK, "reps": args.reps,
           "raw_bytes": int(vol.nbytes), "labels": int(len(np.unique(vol[::4, ::4, ::4])))}

    # ---- encode / decode / copy, everything resident --------------------------------------------------------
    bound = _native.label_encode_bound(8, shape, chunk)
    nchunks = int(np.prod([-(-edge // CHUNK)] * 3))
    d_vol, d_back, d_out = ctx.to_device(vol.reshape(-1)), ctx.alloc(vol.nbytes), ctx.alloc(bound)
    d_off, d_sz = ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    totals = []
    t_enc, all_enc = median_seconds(lambda: totals.append(ctx.label_encode(
        d_vol, 8, shape, chunk, out=d_out, out_capacity=bound, offsets=d_off, sizes=d_sz)), args.reps)
    stored, held = totals[-1]
    assert all(t == totals[0] for t in totals)
    t_dec, all_dec = median_seconds(lambda: ctx.label_decode(d_out, held, d_off, 8, shape, chunk, d_back), args.reps)
    assert np.array_equal(d_back.download(vol.shape, np.uint64), vol), "decode(encode(v)) != v"
    sizes = d_sz.download((nchunks,), np.uint32)
    for d in (d_vol, d_back, d_out, d_off, d_sz):
        d.free()
    a = torch.from_numpy(vol.view(np.int64)).to("cuda:0")
    b = torch.empty_like(a)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()

    t_copy, all_copy = median_seconds(copy, args.reps)
    del a, b
    torch.cuda.empty_cache()
    res["seconds"] = {"encode": t_enc, "decode": t_dec, "device_copy": t_copy,
                      "encode_all": all_enc, "decode_all": all_dec, "device_copy_all": all_copy}
    # bytes the algorithm needs: encode reads the volume twice (size pass, write pass) and writes the streams;
    # decode reads the streams and writes the volume; the copy reads and writes the volume
    res["bytes"] = {"encode": 2 * vol.nbytes + stored, "decode": vol.nbytes + stored, "device_copy": 2 * vol.nbytes}
    res["bytes_per_second"] = {k: res["bytes"][k] / res["seconds"][k] for k in res["bytes"]}
    res["decode_fraction_of_copy_bound"] = (vol.nbytes / t_dec) / (vol.nbytes / t_copy)
    res["decode_output_bytes_per_second"] = vol.nbytes / t_dec
    res["copy_output_bytes_per_second"] = vol.nbytes / t_copy

    # ---- stored bytes against shuffle + zstd-5 of the same chunks ---------------------------------------------
    res["stored_bytes"] = int(stored)
    res["ratio"] = vol.nbytes / stored
    res["largest_chunk_bytes"], res["smallest_chunk_bytes"] = int(sizes.max()), int(sizes.min())
    if zstd_ref.available():
        t0 = time.perf_counter()
        z = zstd_ref.volume_size(vol, chunk, 5, threads=min(16, os.cpu_count() or 1))
        res["shuffle_zstd5_bytes"], res["shuffle_zstd5_ratio"] = int(z), vol.nbytes / z
        res["shuffle_zstd5_host_seconds"] = time.perf_counter() - t0
        res["zstd_version"] = zstd_ref.version()
    else:
        res["shuffle_zstd5_bytes"] = None

    # ---- patches ----------------------------------------------------------------------------------------------
    store_path = os.path.join(work, "labels_store")
    chunk_store.write_zarr(vol, store_path, (1, 1) + chunk, codec=codec)
    arr = chunk_store.open_zarr(store_path)
    rng = np.random.default_rng(1)
    voxels = rng.integers(0, edge, (args.patches, 3))
    box = (args.patch,) * 3
    mm = np.load(raw_path, mmap_mode="r")

    def store_device():
        p = arr.read_patches(voxels, box, out="device")           # synchronises (the gather's status)
        p.free()

    def memmap_device():
        host = read_label_patches(mm, voxels, box)
        d = ctx.to_device(host)                                     # a synchronous copy
        d.free()

    want = read_label_patches(mm, voxels, box)
    assert np.array_equal(arr.read_patches(voxels, box), want), "store patches != memmap patches"
    paths = {"store_to_device": store_device, "store_to_host": lambda: arr.read_patches(voxels, box),
             "memmap_to_device": memmap_device, "memmap_to_host": lambda: read_label_patches(mm, voxels, box)}
    for fn in paths.values():                                       # warm: files in the page cache, code loaded
        fn()
        fn()
    times = {k: [] for k in paths}
    for _ in range(args.reps):                                      # alternating
        for k, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    arr.read_patches(voxels, box, out="device").free()
    res["patches"] = {"count": args.patches, "patch": args.patch, "bytes": int(want.nbytes),
                      "seconds": {k: float(np.median(v)) for k, v in times.items()},
                      "seconds_all": times, "last_read": arr.last_read}
    res["patches"]["store_over_memmap_to_device"] = \
        res["patches"]["seconds"]["store_to_device"] / res["patches"]["seconds"]["memmap_to_device"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
