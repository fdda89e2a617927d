"""Scoring one validation batch three ways.

usage: python tools/bench_validate.py [batch=32] [edge=64] [reps=7]
pred / target uint16, raw float32, a foreground mask of a few per cent.  Times
  (a) loop_host_s    a loop over ``metrics.evaluate_example`` from host arrays: what a caller had to write
                     before ``evaluate_examples``,
  (b) batch_host_s   ``metrics.evaluate_examples`` from host arrays (one upload per operand),
  (c) batch_device_s ``metrics.evaluate_examples`` from CUDA tensors that already lie in HBM,
each as the median wall time of ``reps`` calls after one warm-up call, with a device synchronisation before the
clock starts and before it stops, and prints one JSON line.  The three ways must agree: (b) and (c) bit for
bit, (a) and (b) in everything but the fp64 summation order of the two MAEs."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))

import torch  # noqa: E402

from aind_exaspim_image_compression.machine_learning import metrics  # noqa: E402


def synth(batch, edge, seed=0):
    rng = np.random.default_rng(seed)
    full = (batch, edge, edge, edge)
    signal = 100.0 + 900.0 * (rng.random(full) < 0.03) * rng.random(full)
    raw = (signal + rng.normal(0.0, 12.0, full) - 100.37).astype(np.float32)
    target = np.rint(signal + rng.normal(0.0, 2.0, full)).clip(0, 65535).astype(np.uint16)
    pred = np.rint(signal + rng.normal(0.0, 3.0, full)).clip(0, 65535).astype(np.uint16)
    return pred, raw, target, signal > 130.0


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    edge = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    host = synth(batch, edge)
    dev = tuple(torch.from_numpy(a).cuda() for a in host)

    def loop():
        return [metrics.evaluate_example(*(a[b] for a in host)) for b in range(batch)]

    a, b, c = loop(), metrics.evaluate_examples(*host), metrics.evaluate_examples(*dev)
    for ra, rb, rc in zip(a, b, c):
        assert rb == rc, "host and device operands disagree"
        for key in ra:
            close = abs(ra[key] - rb[key]) <= 1e-12 * abs(ra[key]) if key.endswith("_mae") else ra[key] == rb[key]
            assert close, (key, ra[key], rb[key])
    out = {"batch": batch, "edge": edge, "reps": reps}
    for name, fn in (("loop_host", loop), ("batch_host", lambda: metrics.evaluate_examples(*host)),
                     ("batch_device", lambda: metrics.evaluate_examples(*dev))):
        med, lo, hi = timed(fn, reps)
        out[name + "_s"] = round(med, 6)
        out[name + "_range_s"] = [round(lo, 6), round(hi, 6)]
    out["loop_over_batch_host"] = round(out["loop_host_s"] / out["batch_host_s"], 2)
    out["loop_over_batch_device"] = round(out["loop_host_s"] / out["batch_device_s"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
