"""Connected-component filtering of foreground seeds: what it costs and what it changes.

usage: python tools/bench_components.py [--dir DIR] [--edge 512] [--runs 10] [--rounds 3] [--out-dir profiles/components]
                                        [--limit SECONDS] [--steps make,label,store,consumers]
The driver (no ``--leg``) touches no GPU itself: it starts every step as a process of its own under
``timeout -k 10``, one after the other, and stops at the first one that fails.  The steps:
  make       the seeded synthetic ``edge``^3 uint16 volume of ``bench_foreground_store.py`` in 64^3 chunks (reused if
             there).
  label      resident labelling and filtering of an ``edge``^3 byte mask, for the seeds of that volume at k = 6 and
             for a random mask of density 0.2, connectivity 26: after two warm-ups ``runs`` timings between two events
             of one ``label_components`` call (labels, sizes, kept mask, counters; scratch allocated before); against ``scipy.ndimage.label`` + ``bincount`` + the filter on the host
             (one run, where scipy is importable), and whether the two kept masks agree.
  store      ``foreground_store`` with the volume's measurement passed (one pass), ``dilate = 1``, a budget of 1 GiB,
             at ``min_voxels`` absent, 0, 8, 27 and 64: one warm-up, the median of ``rounds`` runs, seconds per phase,
             ``voxels_read / n`` beside ``(1 + 2 halo / brick)^3`` per axis of the plan's first brick, and the counters.
  consumers  ``n_fg`` and the stored bytes of ``recode_store(codec=BlockBoundedCodec(delta, delta_fg), mask=...)``
             under the unfiltered mask and under the mask filtered at ``min_voxels = 8``.
Every step prints one JSON line and writes ``<out-dir>/<step>_<edge>.json``.  No time is pass or fail.
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
K, DILATE, FILTER = 6.0, 1, 8
BUDGET = 1 << 30                                            # of the store step: several bricks at 512^3 (7.10: 8)
BOUNDS = ((8, 0), (8, 1))                                   # (delta, delta_fg) of DESIGN.md 7.2b


def store_path(a):
    return os.path.join(a.dir, "ref-%d" % a.edge)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def label_leg(a, ctx):
    from bench_store_read import synth
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.utils.noise import measure_volume
    shape, n = (a.edge,) * 3, a.edge ** 3
    vol = synth(a.edge)
    cut = measure_volume(vol).foreground_cut(K)
    masks = {"seeds at k = 6": vol >= cut, "random 0.2": np.random.default_rng(0).random(shape) < 0.2}
    del vol
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    out = {"leg": "label", "edge": a.edge, "runs": a.runs, "connectivity": 26, "min_voxels": FILTER, "cut": cut,
           "scipy": ndimage is not None, "masks": {}}
    scratch_bytes = _native.components_scratch_bytes(shape)
    d_labels, d_sizes, d_kept = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(n)
    d_scratch, d_counts = ctx.alloc(scratch_bytes), ctx.alloc(24)
    e0, e1 = ctx.event(), ctx.event()
    for name, mask in masks.items():
        d_mask = ctx.to_device(mask.view(np.uint8))

        def call():
            ctx.label_components(d_mask, np.uint8, shape, min_voxels=FILTER, connectivity=26, labels=d_labels,
                                 sizes=d_sizes, kept_u8=d_kept, scratch=d_scratch, counts=d_counts)

        for _ in range(2):
            call()
        ctx.sync()
        ms = []
        for _ in range(a.runs):
            ctx.record(e0)
            call()
            ctx.record(e1)
            ctx.sync()
            ms.append(ctx.elapsed_ms(e0, e1))
        seeds, kept, dropped = (int(c) for c in d_counts.download((3,), np.uint64))
        row = {"density": round(float(mask.mean()), 5), "device": spread(ms), "seeds": seeds, "kept": kept,
               "dropped_components": dropped}
        if ndimage is not None:
            t0 = time.perf_counter()
            lab, count = ndimage.label(mask, ndimage.generate_binary_structure(3, 3))
            t1 = time.perf_counter()
            sizes = np.bincount(lab.reshape(-1))
            t2 = time.perf_counter()
            big = sizes >= FILTER
            big[0] = False
            keep = big[lab]
            t3 = time.perf_counter()
            got = d_kept.download(shape, np.uint8).view(bool)
            row.update(host_label_s=round(t1 - t0, 3), host_bincount_s=round(t2 - t1, 3), host_filter_s=round(t3 - t2, 3),
                       host_over_device=round((t3 - t0) * 1e3 / statistics.median(ms), 1), components=int(count),
                       kept_masks_equal=bool(np.array_equal(got, keep)),
                       dropped_equal=bool(dropped == int((sizes[1:] < FILTER).sum())))
            del lab, keep, got
        out["masks"][name] = row
        d_mask.free()
    print(json.dumps(out), flush=True)


def store_leg(a, ctx):
    from aind_exaspim_image_compression.machine_learning import metrics
    from aind_exaspim_image_compression.utils import noise
    from aind_exaspim_image_compression.utils.store_foreground import plan_foreground
    n, src = a.edge ** 3, store_path(a)
    measure = noise.measure_store(src)
    dst = os.path.join(a.dir, "fg-components-%d" % a.edge)
    out = {"leg": "store", "edge": a.edge, "rounds": a.rounds, "k": K, "dilate": DILATE, "runs": {}}
    for name, kw in [("absent", {}), ("0", dict(min_voxels=0)), ("8", dict(min_voxels=8)), ("27", dict(min_voxels=27)),
                     ("64", dict(min_voxels=64))]:
        def run(stats=None):
            return metrics.foreground_store(src, dst, k=K, dilate=DILATE, measure=measure, chunks=CHUNKS, stats=stats,
                                            budget_bytes=BUDGET, **kw)

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
        halo = DILATE + max(0, kw.get("min_voxels", 0) - 1)
        brick = plan_foreground((a.edge,) * 3, CHUNKS[2:], DILATE, BUDGET, kw.get("min_voxels", 0))[0].extent
        out["runs"][name] = {"s": round(statistics.median(secs), 3), "all_s": [round(s, 3) for s in secs],
                             "phases_s": {k: round(v, 4) for k, v in stats["seconds"].items()},
                             "bricks": stats["bricks"], "voxels_read_over_n": round(stats["voxels_read"] / n, 4),
                             "halo": halo, "brick": list(brick),
                             "halo_volume_ratio": round(float(np.prod([1 + 2 * halo / e for e in brick])), 4),
                             "largest_alloc": stats["largest_alloc"],
                             **{k: res[k] for k in ("n_seed", "n_kept", "n_dropped_components", "n_fg")}}
    print(json.dumps(out), flush=True)


def consumers_leg(a, ctx):
    from aind_exaspim_image_compression.machine_learning import metrics
    from aind_exaspim_image_compression.utils import noise, store_recode
    from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
    n, src = a.edge ** 3, store_path(a)
    measure = noise.measure_store(src)
    out = {"leg": "consumers", "edge": a.edge, "k": K, "dilate": DILATE, "masks": {}}
    for name, kw in (("unfiltered", {}), ("min_voxels %d" % FILTER, dict(min_voxels=FILTER))):
        mask = os.path.join(a.dir, "mask-%s-%d" % (name.replace(" ", "-"), a.edge))
        res = metrics.foreground_store(src, mask, k=K, dilate=DILATE, measure=measure, chunks=CHUNKS, **kw)
        row = {k: res[k] for k in ("n_seed", "n_kept", "n_dropped_components", "n_fg")}
        for delta, delta_fg in BOUNDS:
            ratio = store_recode.recode_store(src, os.path.join(a.dir, "recoded-%d" % a.edge),
                                              codec=BlockBoundedCodec(delta, delta_fg), mask=mask, chunks=CHUNKS)
            row["stored_bytes_delta_%d_fg_%d" % (delta, delta_fg)] = int(round(2 * n / ratio))
        out["masks"][name] = row
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
    {"label": label_leg, "store": store_leg, "consumers": consumers_leg}[a.leg](a, _native.context())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10, help="timings of the labelling call (at least 10)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "components"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--leg", choices=("make", "label", "store", "consumers"), default=None)
    ap.add_argument("--steps", default="make,label,store,consumers", help="the steps the driver runs")
    a = ap.parse_args()
    a.runs = max(10, a.runs)
    if a.leg is not None:
        leg(a)
        return
    a.dir = a.dir or tempfile.mkdtemp(prefix="components_")
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir",
               a.dir, "--edge", str(a.edge), "--runs", str(a.runs), "--rounds", str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not lines:
            print("step %s ended with status %d: stopping" % (name, done.returncode), flush=True)
            sys.exit(done.returncode or 1)
        print(lines[-1], flush=True)
        if name != "make":
            with open(os.path.join(a.out_dir, "%s_%d.json" % (name, a.edge)), "w") as f:
                json.dump(json.loads(lines[-1]), f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
