"""The foreground mask of a store against what the whole-volume kernels can do for the same mask.

usage: python tools/bench_foreground_store.py [--dir DIR] [--edge 512] [--runs 11] [--rounds 3] [--out FILE.json]
                                              [--limit SECONDS]
The driver (no ``--leg``) touches no GPU itself: it starts every step as a process of its own under
``timeout -k 10``, one after the other, and stops at the first one that fails.  The steps:
  make     a seeded synthetic ``edge``^3 uint16 volume (``bench_store_read.synth``) written with ``ExacCodec(2)`` in
           64^3 chunks; an existing store under DIR is reused.
  kernel   case A, on the resident volume, for radius 1 and 2, after warm-up, ``runs`` alternating timings between two
           events on the context's stream of
             foreground   one ``foreground_box_u16`` call on the whole volume: threshold, packing, ``radius``
                          iterations, a uint16 mask written;
             dilate       ``ctx.binary_dilate`` with ``radius`` iterations on a byte mask of the volume that is already
                          thresholded -- what the whole-volume kernels offer for the same mask, and LESS work: no
                          threshold, bytes instead of uint16 in and out;
           median, min and max of each, their ratio, and whether the two masks agree.
  store    case B, on the store, after one warm-up of each route, ``rounds`` alternating runs of
             baseline     ``read_zarr`` + ``make_foreground_mask`` + ``write_zarr`` of the mask;
             candidate    ``foreground_store`` (no measurement passed: two passes) in at least 8 bricks;
           medians, one more candidate run with ``stats`` for the phases, and whether the two stores agree file for file.
Every step prints one JSON line; ``--out`` receives one JSON document with the steps.  No time is pass or fail.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNKS = (1, 1, 64, 64, 64)
K = 6.0


def store_path(a):
    return os.path.join(a.dir, "ref-%d" % a.edge)          # the store of bench_compare_stores.py, and shares its name


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def bricks_budget(edge, dilate, least=8):
    """The largest budget, halved from foreground_store's default, whose plan has at least ``least`` bricks."""
    from aind_exaspim_image_compression.utils.store_foreground import plan_foreground
    budget = 4 << 30
    while len(plan_foreground((edge,) * 3, CHUNKS[2:], dilate, budget)) < least and budget > 1:
        budget //= 2
    return budget


def kernel_leg(a, ctx):
    from bench_store_read import synth
    from aind_exaspim_image_compression.utils.noise import measure_volume
    shape, n = (a.edge,) * 3, a.edge ** 3
    vol = synth(a.edge)
    cut = measure_volume(vol).foreground_cut(K)
    out = {"leg": "kernel", "edge": a.edge, "runs": a.runs, "k": K, "cut": cut, "seed_fraction": float((vol >= cut).mean())}
    d_vol = ctx.to_device(vol)
    d_seed = ctx.to_device((vol >= cut).astype(np.uint8))
    d_mask16, d_mask8 = ctx.alloc(2 * n), ctx.alloc(n)
    e0, e1 = ctx.event(), ctx.event()
    for radius in (1, 2):
        calls = {"foreground": lambda: ctx.foreground_box_u16(d_vol, shape, (0, 0, 0), shape, (0, 0, 0), shape, cut,
                                                              radius, 1, out_u16=d_mask16),
                 "dilate": lambda: ctx.binary_dilate(d_seed, 1, shape, radius, d_mask8)}
        for _ in range(3):
            for fn in calls.values():
                fn()
        ctx.sync()
        ms = {name: [] for name in calls}
        for _ in range(a.runs):
            for name, fn in calls.items():                               # alternating
                ctx.record(e0)
                fn()
                ctx.record(e1)
                ctx.sync()
                ms[name].append(ctx.elapsed_ms(e0, e1))
        same = np.array_equal(d_mask16.download(shape, np.uint16) != 0, d_mask8.download(shape, np.uint8) != 0)
        f, d = statistics.median(ms["foreground"]), statistics.median(ms["dilate"])
        out["radius_%d" % radius] = {"foreground": spread(ms["foreground"]), "dilate": spread(ms["dilate"]),
                                     "foreground_over_dilate": round(f / d, 4),
                                     "foreground_GBps": round(4 * n / f / 1e6, 1), "masks_equal": bool(same)}
    print(json.dumps(out), flush=True)


def same_files(a, b):
    def files(root):
        return {os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs}
    if files(a) != files(b):
        return False
    return all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in files(a))


def store_leg(a, ctx):
    from aind_exaspim_image_compression.machine_learning import metrics
    from aind_exaspim_image_compression.utils import chunk_store
    n, dilate = a.edge ** 3, 1
    src = store_path(a)
    budget = bricks_budget(a.edge, dilate)
    dst = {name: os.path.join(a.dir, "fg-%s-%d" % (name, a.edge)) for name in ("baseline", "candidate")}

    def baseline():
        vol = chunk_store.read_zarr(src)[0, 0]
        chunk_store.write_zarr(metrics.make_foreground_mask(vol, K, dilate).astype(np.uint16), dst["baseline"], CHUNKS)

    def candidate(stats=None):
        return metrics.foreground_store(src, dst["candidate"], k=K, dilate=dilate, chunks=CHUNKS, budget_bytes=budget,
                                        stats=stats)

    routes = {"baseline": baseline, "candidate": candidate}
    for run in routes.values():                                          # warm-up: code objects, file cache
        run()
    ctx.sync()
    host_s = {name: [] for name in routes}
    for _ in range(a.rounds):
        for name, run in routes.items():                                 # alternating; both end synchronised
            t0 = time.perf_counter()
            run()
            ctx.sync()
            host_s[name].append(time.perf_counter() - t0)
    stats = {}
    res = candidate(stats)
    b_s, c_s = statistics.median(host_s["baseline"]), statistics.median(host_s["candidate"])
    out = {"leg": "store", "edge": a.edge, "rounds": a.rounds, "budget_bytes": budget, "k": K, "dilate": dilate,
           "bricks": stats["bricks"], "passes": stats["passes"], "voxels_read_over_n": round(stats["voxels_read"] / n, 4),
           "baseline_s": round(b_s, 3), "candidate_s": round(c_s, 3), "candidate_over_baseline": round(c_s / b_s, 4),
           "baseline_host_s": [round(v, 3) for v in host_s["baseline"]],
           "candidate_host_s": [round(v, 3) for v in host_s["candidate"]],
           "phases_s": {k: round(v, 4) for k, v in stats["seconds"].items()},
           "largest_alloc": stats["largest_alloc"], "baseline_device_bytes": 2 * n, "cut": res["cut"],
           "fraction": res["fraction"], "cratio": round(res["cratio"], 2),
           "stores_equal": bool(same_files(dst["baseline"], dst["candidate"]))}
    print(json.dumps(out), flush=True)


def leg(a):
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    if a.leg == "make":
        from bench_store_read import synth
        if not os.path.exists(os.path.join(store_path(a), "zarr.json")):
            chunk_store.write_zarr(synth(a.edge), store_path(a), chunks=CHUNKS, codec=ExacCodec(2))
        print(json.dumps({"leg": "make", "edge": a.edge}), flush=True)
        return
    ctx = _native.context()
    (kernel_leg if a.leg == "kernel" else store_leg)(a, ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--runs", type=int, default=11, help="timings of each kernel (at least 10)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--leg", choices=("make", "kernel", "store"), default=None)
    ap.add_argument("--steps", default="make,kernel,store", help="the steps the driver runs")
    a = ap.parse_args()
    a.runs = max(10, a.runs)
    if a.leg is not None:
        leg(a)
        return
    root = a.dir or tempfile.mkdtemp(prefix="foreground_store_")
    doc = {}
    for name in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir",
               root, "--edge", str(a.edge), "--runs", str(a.runs), "--rounds", str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not lines:
            print("step %s ended with status %d: stopping" % (name, done.returncode), flush=True)
            sys.exit(done.returncode or 1)
        print(lines[-1], flush=True)
        doc[name] = json.loads(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
