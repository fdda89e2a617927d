"""Labelling the components of a store out of core: what it costs, phase by phase.

usage: python tools/bench_components_store.py [--dir DIR] [--edge 512] [--bricks 8] [--rounds 3]
                                              [--out profiles/segment/components_store_512.json]
                                              [--inputs seeds,random] [--no-scipy]
One process; run it under ``timeout``.  For the seeds of the synthetic ``edge``^3 volume of ``bench_store_read.synth``
at k = 6 and for a random mask of density 0.2 (the inputs of ``tools/bench_components.py``), each written as a uint16
store in 64^3 chunks, connectivity 26, uint32 labels:
  store      ``components_store`` under the smallest budget (a multiple of 64 MiB) at which ``plan_segment`` makes at
             most ``--bricks`` bricks: one warm-up, the median of ``rounds`` unsynchronised runs, then one run with
             ``stats`` for the seconds per phase, the records and ``largest_alloc``.
  in_memory  the path the parent commit offers: ``read_zarr`` + ``label_components`` of the whole array + ``write_zarr``
             with ``LabelCodec(4)``, and whether its chunk files equal the store path's.
  scipy      ``scipy.ndimage.label`` of the mask on the host (one run, where scipy is importable).
Prints one JSON line and writes ``--out``.  No time is pass or fail.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNKS = (1, 1, 64, 64, 64)
K = 6.0


def chunk_files(path):
    found = {}
    for root, _, files in os.walk(os.path.join(path, "c")):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                found[os.path.relpath(os.path.join(root, f), path)] = fh.read()
    return found


def budget_for(shape, bricks):
    from aind_exaspim_image_compression.utils.store_segment import plan_segment
    budget = 64 << 20
    while len(plan_segment(shape, CHUNKS[2:], budget, 4)) > bricks:
        budget += 64 << 20
    return budget


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--bricks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--inputs", default="seeds,random")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    from bench_store_read import synth
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.machine_learning import metrics
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.label_codec import LabelCodec
    from aind_exaspim_image_compression.utils.noise import measure_volume
    from aind_exaspim_image_compression.utils.store_segment import plan_segment
    ndimage = None
    if not a.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            pass
    work = a.dir or tempfile.mkdtemp(prefix="components-store-")
    os.makedirs(work, exist_ok=True)
    shape, n = (a.edge,) * 3, a.edge ** 3
    ctx = _native.context()
    budget = budget_for(shape, a.bricks)
    plan = plan_segment(shape, CHUNKS[2:], budget, 4)
    out = {"edge": a.edge, "connectivity": 26, "rounds": a.rounds, "budget_bytes": budget, "bricks": len(plan),
           "brick": list(plan[0].extent), "scipy": ndimage is not None, "inputs": {}}
    for name in a.inputs.split(","):
        if name == "seeds":
            vol = synth(a.edge)
            threshold = measure_volume(vol).foreground_cut(K) - 1      # cut = floor(threshold) + 1
        else:
            vol = (np.random.default_rng(0).random(shape) < 0.2).astype(np.uint16)
            threshold = 0
        src, dst, ref = (os.path.join(work, "%s-%s-%d" % (name, what, a.edge)) for what in ("src", "labels", "ref"))
        chunk_store.write_zarr(vol, src, chunks=CHUNKS)
        mask = vol > threshold
        del vol

        def run(stats=None):
            return metrics.components_store(src, dst, threshold=threshold, connectivity=26, chunks=CHUNKS,
                                            budget_bytes=budget, stats=stats)

        run()
        ctx.sync()
        secs = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            run()
            ctx.sync()
            secs.append(time.perf_counter() - t0)
        stats = {}
        res = run(stats)
        row = {"density": round(float(mask.mean()), 5), "cut": res["cut"],
               "store": {"s": round(statistics.median(secs), 3), "all_s": [round(s, 3) for s in secs],
                         "phases_s": {k: round(v, 4) for k, v in stats["seconds"].items()},
                         "records": stats["records"], "collect_repeats": stats["collect_repeats"],
                         "voxels_read_over_n": round(stats["voxels_read"] / n, 4),
                         "largest_alloc": stats["largest_alloc"], "cratio": round(res["cratio"], 2),
                         **{k: res[k] for k in ("n_seed", "n_components", "largest")}}}
        # the in-memory path of the parent commit
        t0 = time.perf_counter()
        whole = chunk_store.read_zarr(src)[0, 0]
        t1 = time.perf_counter()
        labels, count = metrics.label_components(whole > threshold, 26)
        t2 = time.perf_counter()
        chunk_store.write_zarr(labels.view(np.uint32), ref, chunks=CHUNKS, codec=LabelCodec(4))
        t3 = time.perf_counter()
        row["in_memory"] = {"s": round(t3 - t0, 3), "read_zarr_s": round(t1 - t0, 3),
                            "label_components_s": round(t2 - t1, 3), "write_zarr_s": round(t3 - t2, 3),
                            "components": int(count), "files_equal": chunk_files(dst) == chunk_files(ref)}
        del whole, labels
        if ndimage is not None:
            t0 = time.perf_counter()
            _, count = ndimage.label(mask, ndimage.generate_binary_structure(3, 3))
            row["scipy"] = {"label_s": round(time.perf_counter() - t0, 3), "components": int(count)}
        out["inputs"][name] = row
        print(json.dumps({name: row}), flush=True)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
