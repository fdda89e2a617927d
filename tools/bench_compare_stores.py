"""Scoring one store against another out of core against the whole-volume route.

usage: python tools/bench_compare_stores.py [--dir DIR] [--edge 512] [--rounds 3] [--out FILE.json] [--limit SECONDS]
The driver (no ``--leg``) touches no GPU itself: it starts every step as a process of its own under
``timeout -k 10``, one after the other, and stops at the first one that fails.  The steps:
  make       a seeded synthetic ``edge``^3 uint16 volume (``bench_store_read.synth``) written with ``ExacCodec(2)``
             and, as the store to score, with ``BoundedDctCodec(8)``, both in 64^3 chunks (existing stores under DIR
             are reused);
  run        in one process, after one warm-up of each, ``rounds`` alternating runs of
               baseline   what could be done before ``compare_stores``: ``read_zarr`` of both stores, then ``ssim3D``,
                          ``compute_mae`` and ``compute_lmax`` on the arrays and the nine projections with numpy;
               candidate  ``compare_stores`` with the same ``data_range`` given (one pass), at the largest budget,
                          halved from the default, that gives at least 8 bricks;
             each between two events on the context's stream (the host clock is recorded next to them), medians
             reported, and one more candidate run with ``stats`` for the phases.
The ``run`` step prints one JSON line (written to ``--out``): both medians, their ratio, ``voxels_read / n``, the
bound ``baseline x voxels_read / n x 1.1`` the candidate is held to (the halo re-read is the only extra work it does;
10 % for per-brick launches and synchronisation) and whether it holds, the phases and ``largest_alloc``.  The two routes'
numbers are compared (equal but for the SSIM's summation order).  No time is pass or fail.
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
DELTA = 8
WINDOW = 16


def bricks_budget(edge, least=8):
    """The largest budget, halved from compare_stores' default, whose plan has at least ``least`` bricks."""
    from aind_exaspim_image_compression.utils.store_compare import plan_compare
    budget = 4 << 30
    while len(plan_compare((edge,) * 3, CHUNKS[2:], WINDOW, budget)) < least and budget > 1:
        budget //= 2
    return budget


def baseline(ref_path, test_path, data_range):
    from aind_exaspim_image_compression.utils import chunk_store, img_util
    a = chunk_store.read_zarr(ref_path)[0, 0]
    b = chunk_store.read_zarr(test_path)[0, 0]
    out = {"ssim": float(img_util.ssim3D(a, b, data_range=data_range, window_size=WINDOW)),
           "mae": img_util.compute_mae(a, b), "lmax": img_util.compute_lmax(a, b)}
    diff = np.abs(b.astype(np.int32) - a.astype(np.int32))
    out["mips"] = {name: tuple(np.max(v, axis=axis) for axis in range(3))
                   for name, v in (("ref", a), ("test", b), ("abs_diff", diff))}
    return out


def leg(a):
    from aind_exaspim_image_compression import _native, evaluate
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    from bench_store_read import synth
    ref_path = os.path.join(a.dir, "ref-%d" % a.edge)
    test_path = os.path.join(a.dir, "bounded-%d" % a.edge)
    if a.leg == "make":
        if not (os.path.exists(os.path.join(ref_path, "zarr.json")) and
                os.path.exists(os.path.join(test_path, "zarr.json"))):
            vol = synth(a.edge)
            chunk_store.write_zarr(vol, ref_path, chunks=CHUNKS, codec=ExacCodec(2))
            chunk_store.write_zarr(vol, test_path, chunks=CHUNKS, codec=BoundedDctCodec(DELTA))
        print(json.dumps({"leg": "make", "edge": a.edge}), flush=True)
        return

    ctx = _native.context()
    n = a.edge ** 3
    budget = bricks_budget(a.edge)
    data_range = 1000.0
    routes = {"baseline": lambda: baseline(ref_path, test_path, data_range),
              "candidate": lambda: evaluate.compare_stores(ref_path, test_path, data_range=data_range,
                                                           window_size=WINDOW, budget_bytes=budget)}
    results = {name: run() for name, run in routes.items()}             # warm-up: code objects, file cache
    ctx.sync()
    event_ms = {name: [] for name in routes}
    host_s = {name: [] for name in routes}
    for _ in range(a.rounds):
        for name, run in routes.items():                                 # alternating
            e0, e1 = ctx.event(), ctx.event()
            ctx.record(e0)
            t0 = time.perf_counter()
            run()
            ctx.record(e1)
            ctx.sync()
            host_s[name].append(time.perf_counter() - t0)
            event_ms[name].append(ctx.elapsed_ms(e0, e1))
    stats = {}
    evaluate.compare_stores(ref_path, test_path, data_range=data_range, window_size=WINDOW, budget_bytes=budget,
                            stats=stats)
    base, cand = results["baseline"], results["candidate"]
    same = (base["mae"] == cand["mae"] and base["lmax"] == cand["lmax"] and
            all(np.array_equal(base["mips"][k][ax], cand["mips"][k][ax]) for k in base["mips"] for ax in range(3)))
    b_s = statistics.median(event_ms["baseline"]) / 1e3
    c_s = statistics.median(event_ms["candidate"]) / 1e3
    reread = stats["voxels_read"] / n
    out = {"leg": "run", "edge": a.edge, "window": WINDOW, "max_error": DELTA, "rounds": a.rounds,
           "budget_bytes": budget, "bricks": stats["bricks"], "voxels_read_over_n": round(reread, 4),
           "baseline_s": round(b_s, 3), "candidate_s": round(c_s, 3), "candidate_over_baseline": round(c_s / b_s, 4),
           "bound_s": round(1.1 * reread * b_s, 3), "within_bound": bool(c_s <= 1.1 * reread * b_s),
           "baseline_event_s": [round(v / 1e3, 3) for v in event_ms["baseline"]],
           "candidate_event_s": [round(v / 1e3, 3) for v in event_ms["candidate"]],
           "baseline_host_s": [round(v, 3) for v in host_s["baseline"]],
           "candidate_host_s": [round(v, 3) for v in host_s["candidate"]],
           "phases_s": {k: round(v, 3) for k, v in stats["seconds"].items()},
           "largest_alloc": stats["largest_alloc"], "baseline_device_bytes": 2 * 2 * n,
           "mae": cand["mae"], "lmax": cand["lmax"], "ssim_candidate": cand["ssim"], "ssim_baseline": base["ssim"],
           "ssim_difference": abs(cand["ssim"] - base["ssim"]), "exact_results_equal": bool(same),
           "cratio_ref": round(cand["cratio_ref"], 3), "cratio_test": round(cand["cratio_test"], 3)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--leg", choices=("make", "run"), default=None)
    a = ap.parse_args()
    if a.leg is not None:
        leg(a)
        return
    root = a.dir or tempfile.mkdtemp(prefix="compare_stores_")
    for name in ("make", "run"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir",
               root, "--edge", str(a.edge), "--rounds", str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not lines:
            print("step %s ended with status %d: stopping" % (name, done.returncode), flush=True)
            sys.exit(done.returncode or 1)
        print(lines[-1], flush=True)
        if a.out and name == "run":
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(json.loads(lines[-1]), indent=1) + "\n")


if __name__ == "__main__":
    main()
