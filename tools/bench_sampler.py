"""Drawing training patches out of a local store.

usage: python tools/bench_sampler.py [tasks=256] [edge=512] [patch=64] [reps=3] [--trace-run]
Writes a seeded synthetic ``edge``^3 uint16 volume (background, noise, bright tubes) as a chunk store in a
temporary directory -- a brain with neither labels nor a skeleton, so every foreground draw is a
``sample_bright_voxel`` search -- and times, teacher left out (BM4D is the same work on both sides):

  batched   ``PatchSampler.sample_counts`` of all tasks, the candidates of a round scored in one device pass
  serial    the same tasks one by one through the single-draw methods (``sample_task``): the reference's shape of
            work on this repository's per-patch calls

Both are warmed once, then timed ``reps`` times alternating, a host clock around work that ends in a
synchronisation; the two results are asserted equal before anything is timed.  Prints one JSON line with the
medians (min, max).  ``--trace-run``: the batched form only, ``reps`` times and untimed, for a
``rocprofv3 --kernel-trace --stats`` run of its own."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))

from aind_exaspim_image_compression.machine_learning import sampling  # noqa: E402
from aind_exaspim_image_compression.utils import chunk_store  # noqa: E402


def synth(edge, seed=0):
    rng = np.random.default_rng(seed)
    vol = rng.normal(100.0, 6.0, (edge,) * 3).astype(np.float32)
    y, x = np.meshgrid(np.arange(edge, dtype=np.float32), np.arange(edge, dtype=np.float32), indexing="ij")
    for _ in range(edge // 8):
        cy, cx = rng.uniform(0, edge, 2)
        tube = (400.0 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / 4.0)).astype(np.float32)
        z0 = int(rng.integers(0, edge - 32))
        vol[z0:z0 + 32] += tube
    return np.clip(np.rint(vol), 0, 65535).astype(np.uint16)


def stats(ts):
    return {"median_s": round(float(np.median(ts)), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}


def main():
    trace = "--trace-run" in sys.argv
    args = [int(a) for a in sys.argv[1:] if a != "--trace-run"]
    tasks, edge, patch, reps = args + [256, 512, 64, 3][len(args):]
    with tempfile.TemporaryDirectory() as root:
        path = os.path.join(root, "brain")
        chunk_store.write_zarr(synth(edge), path, (1, 1, 64, 64, 64))
        src = {"brain": sampling.BrainSource(chunk_store.open_zarr(path), offset=37.0)}
        sampler = sampling.PatchSampler(src, (patch,) * 3, boundary_buffer=patch)
        idx = list(range(tasks))

        def batched():
            return sampler.sample_counts(idx, 42, "train", batch_tasks=tasks, teacher=False)

        def serial():
            return [sampler.sample_task(i, 42, "train", teacher=False) for i in idx]

        if trace:
            for _ in range(reps):
                batched()
            return
        got, one = batched(), serial()                    # warm-up, and the two must agree
        assert all(tuple(got[1][i]) == tuple(one[i][1]) for i in idx)
        assert all(np.array_equal(got[2][i], one[i][2]) and np.array_equal(got[4][i], one[i][4]) for i in idx)
        tb, ts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            batched()
            t1 = time.perf_counter()
            serial()
            t2 = time.perf_counter()
            tb.append(t1 - t0)
            ts.append(t2 - t1)
            print(f"batched {tb[-1]:.3f} s, serial {ts[-1]:.3f} s", file=sys.stderr, flush=True)
    print(json.dumps({"tasks": tasks, "edge": edge, "patch": patch, "reps": reps, "batched": stats(tb),
                      "serial": stats(ts), "batched_patches_per_s": round(tasks / float(np.median(tb)), 1),
                      "serial_patches_per_s": round(tasks / float(np.median(ts)), 1),
                      "ratio": round(float(np.median(ts)) / float(np.median(tb)), 2)}))


if __name__ == "__main__":
    main()
