"""Measuring a store out of core against the whole-volume kernels and the in-memory route.

usage: python tools/bench_measure_store.py [--dir DIR] [--edge 512] [--runs 11] [--rounds 3] [--out FILE.jsonl]
                                           [--limit SECONDS]
The driver (no ``--leg``) touches no GPU itself: it starts every step as a process of its own under
``timeout -k 10``, one after the other, and stops at the first one that fails.  The steps:
  make     two seeded synthetic ``edge``^3 uint16 volumes written with ``ExacCodec(2)`` in 64^3 chunks: ``quiet``
           (``bench_store_read.synth``, the store of ``bench_compare_stores.py``; the noise table needs shift 0) and
           ``loud`` (30000 + N(0, 9000): the in-memory rule repeats its pass up to shift 3).  Existing stores under DIR
           are reused.
  kernel   on the resident ``quiet`` volume, after warm-up, ``runs`` alternating timings between two events on the
           context's stream of
             measure     one ``measure_box_u16`` call on the whole volume (zeroing included, tables left on the device);
             measure+dl  the same and the download of both tables;
             histogram   ``ctx.u16_histogram``    } the two kernels it replaces, each with its zeroing and its copy of
             noise       ``ctx.noise_table(0)``   } the table to the host;
           median, min and max of each, and of histogram + noise run by run; and the same four on the ``loud`` volume,
           where nothing fits the tables kept in LDS.
  store    on each store, after one warm-up of each route, ``rounds`` alternating runs of
             baseline    ``read_zarr``, then ``estimate_offset`` and ``noise.noise_table`` on the array (the auto rule:
                         one pass on ``quiet``, several on ``loud``);
             candidate   ``measure_store`` in at least 8 bricks, then ``offset()`` and ``noise_table()`` of the result;
           medians, one more candidate run with ``stats`` for the phases, and whether the two routes agree.
Every step prints one JSON line (appended to ``--out``).  No time is pass or fail.
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
KINDS = ("quiet", "loud")


def volume(kind, edge):
    from bench_store_read import synth
    if kind == "quiet":
        return synth(edge)
    rng = np.random.default_rng(3)
    vol = rng.standard_normal((edge, edge, edge), dtype=np.float32) * 9000.0 + 30000.0
    return np.clip(np.rint(vol), 0, 65535).astype(np.uint16)


def store_path(a, kind):
    # ``quiet`` is the reference store of bench_compare_stores.py, and shares its name
    return os.path.join(a.dir, ("ref-%d" if kind == "quiet" else "loud-%d") % a.edge)


def bricks_budget(edge, least=8):
    """The largest budget, halved from measure_store's default, whose plan has at least ``least`` bricks."""
    from aind_exaspim_image_compression.utils.store_measure import plan_measure
    budget = 4 << 30
    while len(plan_measure((edge,) * 3, CHUNKS[2:], budget)) < least and budget > 1:
        budget //= 2
    return budget


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_leg(a, ctx):
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.utils import store_measure
    shape, n = (a.edge,) * 3, a.edge ** 3
    out = {"leg": "kernel", "edge": a.edge, "runs": a.runs}
    d_counts = ctx.alloc(8 * _native.COUNT_BINS)
    d_noise = ctx.alloc(8 * _native.measure_noise_words())
    e0, e1 = ctx.event(), ctx.event()
    for kind in KINDS:
        d_vol = ctx.to_device(volume(kind, a.edge))

        def measure():
            ctx.measure_box_u16(d_vol, None, shape, (0, 0, 0), shape, (0, 0, 0), shape, d_counts, d_noise,
                                zero_first=True)

        def measure_dl():
            measure()
            return (d_counts.download((_native.COUNT_BINS,), np.uint64),
                    d_noise.download((_native.measure_noise_words(),), np.uint64))

        calls = {"measure": measure, "measure_and_download": measure_dl,
                 "u16_histogram": lambda: ctx.u16_histogram(d_vol, n),
                 "noise_table": lambda: ctx.noise_table(d_vol, np.uint16, shape, 0)}
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
        both = [h + t for h, t in zip(ms["u16_histogram"], ms["noise_table"])]
        counts, tab = measure_dl()
        hist, sum_s, _ = ctx.noise_table(d_vol, np.uint16, shape, 0)
        wide = tab[:-_native.NOISE_LEVELS].reshape(_native.NOISE_LEVELS, _native.NOISE_WIDE_BINS)
        same = (np.array_equal(counts, ctx.u16_histogram(d_vol, n)) and np.array_equal(tab[-_native.NOISE_LEVELS:], sum_s)
                and np.array_equal(store_measure.fold_noise_table(wide, 0), hist))
        res = {name: spread(v) for name, v in ms.items()}
        res["histogram_plus_noise"] = spread(both)
        res["measure_over_sum"] = round(statistics.median(ms["measure"]) / statistics.median(both), 4)
        res["measure_and_download_over_sum"] = round(statistics.median(ms["measure_and_download"]) /
                                                     statistics.median(both), 4)
        res["measure_GBps"] = round(2 * n / statistics.median(ms["measure"]) / 1e6, 1)
        res["tables_equal"] = bool(same)
        res["values_beyond_the_band"] = int(counts[8192:].sum())
        res["cells_in_wide_bins_from_4096"] = int(wide[:, 4096:].sum())
        res["levels_populated"] = int(np.count_nonzero(wide.sum(axis=1)))
        out[kind] = res
        d_vol.free()
    print(json.dumps(out), flush=True)


def store_leg(a, ctx):
    from aind_exaspim_image_compression.machine_learning.transforms import estimate_offset
    from aind_exaspim_image_compression.utils import chunk_store, noise
    n = a.edge ** 3
    budget = bricks_budget(a.edge)
    out = {"leg": "store", "edge": a.edge, "rounds": a.rounds, "budget_bytes": budget}
    for kind in KINDS:
        path = store_path(a, kind)

        def baseline():
            vol = chunk_store.read_zarr(path)[0, 0]
            return estimate_offset(vol), noise.noise_table(vol)

        def candidate():
            m = noise.measure_store(path, budget_bytes=budget)
            return m.offset(), m.noise_table()

        routes = {"baseline": baseline, "candidate": candidate}
        results = {name: run() for name, run in routes.items()}          # warm-up: code objects, file cache
        ctx.sync()
        host_s = {name: [] for name in routes}
        for _ in range(a.rounds):
            for name, run in routes.items():                             # alternating; both end synchronised
                t0 = time.perf_counter()
                run()
                ctx.sync()
                host_s[name].append(time.perf_counter() - t0)
        stats = {}
        t0 = time.perf_counter()
        m = noise.measure_store(path, budget_bytes=budget, stats=stats)
        t1 = time.perf_counter()
        m.offset(), m.noise_table()
        t2 = time.perf_counter()
        (b_off, b_tab), (c_off, c_tab) = results["baseline"], results["candidate"]
        same = (b_off == c_off and b_tab.shift == c_tab.shift and np.array_equal(b_tab.hist, c_tab.hist) and
                np.array_equal(b_tab.sum_s, c_tab.sum_s))
        b_s, c_s = statistics.median(host_s["baseline"]), statistics.median(host_s["candidate"])
        total = sum(stats["seconds"].values())
        out[kind] = {"bricks": stats["bricks"], "voxels_read_over_n": round(stats["voxels_read"] / n, 4),
                     "shift": int(c_tab.shift), "baseline_passes_over_the_array": int(b_tab.shift) + 1,
                     "baseline_s": round(b_s, 3), "candidate_s": round(c_s, 3),
                     "candidate_over_baseline": round(c_s / b_s, 4),
                     "baseline_host_s": [round(v, 3) for v in host_s["baseline"]],
                     "candidate_host_s": [round(v, 3) for v in host_s["candidate"]],
                     "phases_s": {k: round(v, 4) for k, v in stats["seconds"].items()},
                     "read_share_of_phases": round(stats["seconds"]["read"] / total, 4),
                     "timed_run_s": round(t1 - t0, 3), "host_estimators_s": round(t2 - t1, 4),
                     "largest_alloc": stats["largest_alloc"], "baseline_device_bytes": 2 * n,
                     "offset": c_off, "sigma": c_tab.pooled_sigma(), "results_equal": bool(same)}
    print(json.dumps(out), flush=True)


def leg(a):
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    if a.leg == "make":
        for kind in KINDS:
            path = store_path(a, kind)
            if not os.path.exists(os.path.join(path, "zarr.json")):
                chunk_store.write_zarr(volume(kind, a.edge), path, chunks=CHUNKS, codec=ExacCodec(2))
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
    a = ap.parse_args()
    a.runs = max(10, a.runs)
    if a.leg is not None:
        leg(a)
        return
    root = a.dir or tempfile.mkdtemp(prefix="measure_store_")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for name in ("make", "kernel", "store"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir",
               root, "--edge", str(a.edge), "--runs", str(a.runs), "--rounds", str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not lines:
            print("step %s ended with status %d: stopping" % (name, done.returncode), flush=True)
            sys.exit(done.returncode or 1)
        print(lines[-1], flush=True)
        if a.out and name != "make":
            with open(a.out, "a") as f:
                f.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
