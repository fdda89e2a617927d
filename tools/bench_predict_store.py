"""BM4DNet inference store to store against the whole-volume route.

usage: python tools/bench_predict_store.py [--dir DIR] [--edge 512] [--precisions fp32,fp16] [--out FILE.jsonl]
                                           [--limit SECONDS]
The driver (no ``--leg``) touches no GPU itself: it starts every step as a process of its own under
``timeout -k 10``, one after the other, and stops at the first one that fails.  The steps:
  make       a seeded synthetic ``edge``^3 uint16 volume (``bench_store_read.synth``) written with ``ExacCodec(2)`` in
             64^3 chunks (an existing store under DIR is reused);
and per precision, with the seeded ``UNet()`` and the asinh transform, after a warm-up ``predict`` of 192^3:
  baseline   ``read_zarr`` + ``predict`` + ``write_zarr``, each timed, and ``predict`` with an identity callable: what
             the whole-volume call spends outside its forward passes;
  default    ``predict_store`` at the default budget, once without ``stats`` (the wall time: no synchronisation per
             batch) and once with (the phases);
  bricks     the same at the largest budget, halved from the default, that gives at least 8 bricks.
Every leg prints one JSON line (collected in ``--out``): seconds, the phase table, ``patches_run / patches_unique``,
``largest_alloc``, the share of the call outside ``forward`` and how its files compare with the baseline's.  No time is
pass or fail.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TF_CFG = {"kind": "asinh", "params": {"offset": 0.0, "scale": 32.0}}
CHUNKS = (1, 1, 64, 64, 64)


def files_of(path):
    out = {}
    for root, _, names in os.walk(path):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), path)] = f.read()
    return out


def bricks_budget(edge, batch_size=32, least=8):
    """The largest budget, halved from predict_store's default, whose plan has at least ``least`` bricks."""
    from aind_exaspim_image_compression.utils.store_predict import plan_predict
    budget = 16 << 30
    while len(plan_predict((edge,) * 3, CHUNKS[2:], 64, 12, 5, batch_size, budget)) < least and budget > 1:
        budget //= 2
    return budget


def leg(a):
    import torch
    from aind_exaspim_image_compression import inference
    from aind_exaspim_image_compression.machine_learning import transforms as T
    from aind_exaspim_image_compression.machine_learning import unet3d
    from aind_exaspim_image_compression.utils import chunk_store
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    from bench_store_read import synth
    src = os.path.join(a.dir, "src-%d" % a.edge)
    if a.leg == "make":
        if not os.path.exists(os.path.join(src, "zarr.json")):
            chunk_store.write_zarr(synth(a.edge), src, chunks=CHUNKS, codec=ExacCodec(2))
        print(json.dumps({"leg": "make", "edge": a.edge}), flush=True)
        return
    torch.manual_seed(0)
    model = unet3d.UNet().cuda().eval()
    tf = T.build_transform(TF_CFG)
    inference.predict(synth(192), model, tf, verbose=False, precision=a.precision)        # MIOpen's kernels, loaded
    torch.cuda.synchronize()
    base = os.path.join(a.dir, "baseline-%d-%s" % (a.edge, a.precision))
    out = {"leg": a.leg, "edge": a.edge, "precision": a.precision}

    if a.leg == "baseline":
        t0 = time.perf_counter()
        vol = chunk_store.read_zarr(src)[0, 0]
        t1 = time.perf_counter()
        res = inference.predict(vol, model, tf, verbose=False, precision=a.precision)
        t2 = time.perf_counter()
        chunk_store.write_zarr(res, base, chunks=CHUNKS, codec=ExacCodec(2))
        t3 = time.perf_counter()
        inference.predict(vol, lambda x: x, tf, verbose=False, precision=a.precision)
        t4 = time.perf_counter()
        out.update(seconds=round(t3 - t0, 3), read_zarr_s=round(t1 - t0, 3), predict_s=round(t2 - t1, 3),
                   write_zarr_s=round(t3 - t2, 3), predict_identity_s=round(t4 - t3, 3),
                   predict_outside_forward_share=round((t4 - t3) / (t2 - t1), 4),
                   device_bytes_per_voxel=14, device_bytes=14 * a.edge ** 3)
        print(json.dumps(out), flush=True)
        return

    budget = 16 << 30 if a.leg == "default" else bricks_budget(a.edge)
    dst = os.path.join(a.dir, "%s-%d-%s" % (a.leg, a.edge, a.precision))
    t0 = time.perf_counter()
    inference.predict_store(src, dst, model, tf, verbose=False, precision=a.precision, budget_bytes=budget)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    stats = {}
    t0 = time.perf_counter()
    inference.predict_store(src, dst, model, tf, verbose=False, precision=a.precision, budget_bytes=budget, stats=stats)
    timed = time.perf_counter() - t0
    phases = {k: round(v, 3) for k, v in stats["seconds"].items()}
    out.update(budget_bytes=budget, seconds=round(wall, 3), seconds_with_stats=round(timed, 3), phases_s=phases,
               other_s=round(timed - sum(stats["seconds"].values()), 3),
               outside_forward_share=round(1.0 - stats["seconds"]["forward"] / timed, 4),
               bricks=stats["bricks"], patches_run=stats["patches_run"], patches_unique=stats["patches_unique"],
               seam_share=round(stats["patches_run"] / max(stats["patches_unique"], 1), 4),
               largest_alloc=stats["largest_alloc"])
    if os.path.exists(os.path.join(base, "zarr.json")):
        want, got = files_of(base), files_of(dst)
        differing = sorted(k for k in want if got.get(k) != want[k])
        out.update(files=len(want), files_differing=len(differing))
        if differing:
            d = np.abs(chunk_store.read_zarr(dst)[0, 0].astype(np.int32) -
                       chunk_store.read_zarr(base)[0, 0].astype(np.int32))
            out.update(max_count_difference=int(d.max()), voxels_differing=int(np.count_nonzero(d)))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--precisions", default="fp32,fp16")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--leg", choices=("make", "baseline", "default", "bricks"), default=None)
    a = ap.parse_args()
    if a.leg is not None:
        leg(a)
        return
    root = a.dir or tempfile.mkdtemp(prefix="predict_store_")
    steps = [("make", "fp32")] + [(name, p) for p in a.precisions.split(",")
                                  for name in ("baseline", "default", "bricks")]
    for name, precision in steps:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--dir",
               root, "--edge", str(a.edge), "--precision", precision]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not lines:
            print("step %s %s ended with status %d: stopping" % (name, precision, done.returncode), flush=True)
            sys.exit(done.returncode or 1)
        print(lines[-1], flush=True)
        if a.out and name != "make":
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
