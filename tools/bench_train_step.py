"""One full BM4DNet training step -- forward, loss, backward, AdamW step -- at batch 32 x 64^3 in fp32, in three
configurations, each in a process of its own:
  (a) the plain model, the framework's layout and modules, the torch loss
  (b) the plain model in channels_last_3d, the torch loss
  (c) machine_learning.train.trainable_ndhwc with the device loss
Median of --steps steps after --warmup, timed with device events.  With --trace (needs rocprofv3 on PATH) one more
run of (c) under `rocprofv3 --kernel-trace --stats` gives the share of this repository's kernels in the step's
kernel time.  Appends one JSON line to profiles/train/train_step.jsonl and prints it.  Not part of bench.py."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
OWN_KERNELS = ("gn_", "maxpool2_", "upsample2_", "charbonnier_")


def run_config(config, batch, steps, warmup):
    import torch
    from aind_exaspim_image_compression import inference
    from aind_exaspim_image_compression.machine_learning import losses, train, unet3d

    inference._miopen_defaults()
    torch.manual_seed(0)
    model = unet3d.UNet().cuda()
    net = model
    if config == "b":
        model.to(memory_format=torch.channels_last_3d)
    if config == "c":
        net = train.trainable_ndhwc(model)
        criterion = losses.SignalPreservingLoss()
    else:
        def criterion(pred, target, fg):          # the reference's expression, whatever the layout
            return ((1.0 + 20.0 * fg) * losses.charbonnier(pred - target, 1e-3)).mean()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    x = torch.randn(batch, 1, 64, 64, 64, device="cuda")
    y = x + 0.1 * torch.randn_like(x)
    fg = (torch.rand_like(x) < 0.1).float()
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = train.train_step(net, opt, criterion, x, y, fg)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"config": config, "ms": statistics.median(times), "loss": float(loss),
            "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30}


def child(args, config, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--config", config, "--batch", str(args.batch),
                          "--steps", str(args.steps), "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def kernel_shares(args):
    """Per-kernel share (%) of this repository's kernels in the kernel time of configuration (c)."""
    with tempfile.TemporaryDirectory() as d:
        child(args, "c", prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    own = {}
    for r in rows:
        name = r["Name"].split("(")[0].split("<")[0].replace("void exabm4d::", "").replace("exabm4d::", "")
        if name.startswith(OWN_KERNELS):
            own[name] = own.get(name, 0.0) + 100.0 * float(r["TotalDurationNs"]) / total
    return {k: round(v, 2) for k, v in sorted(own.items(), key=lambda kv: -kv[1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices="abc", help="run one configuration in this process (what the parent starts)")
    ap.add_argument("--trace", action="store_true", help="also trace (c)'s kernels with rocprofv3")
    args = ap.parse_args()
    if args.config:
        print(json.dumps(run_config(args.config, args.batch, args.steps, args.warmup)), flush=True)
        return
    res = {c: child(args, c) for c in "abc"}
    line = {"batch": args.batch, "patch": 64, "dtype": "fp32", "steps": args.steps, "warmup": args.warmup,
            "ms_plain": res["a"]["ms"], "ms_plain_ndhwc": res["b"]["ms"], "ms_trainable_ndhwc": res["c"]["ms"],
            "peak_gib": {c: round(res[c]["peak_gib"], 2) for c in "abc"}}
    if args.trace:
        line["own_kernel_share_percent"] = kernel_shares(args)
    os.makedirs(os.path.join(ROOT, "profiles", "train"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train", "train_step.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
