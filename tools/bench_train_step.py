"""One full BM4DNet training step -- forward, loss, backward, AdamW step -- at batch 32 x 64^3, each configuration
in a process of its own.  In fp32 (--precision fp32, the default):
  (a) the plain model, the framework's layout and modules, the torch loss
  (b) the plain model in channels_last_3d, the torch loss
  (c) machine_learning.train.trainable_ndhwc with the device loss
Under fp16 / bf16 autocast (--precision fp16 | bf16; fp16 with a GradScaler, as the reference trains):
  (d) the plain model in channels_last_3d under the framework's autocast, the torch loss
  (e) trainable_ndhwc(model, precision=...) with the device loss -- the comparison that matters is (e) against (d)
--precision all runs the three fp32 legs and (d), (e) in both half types: seven legs, one JSON line.
Median of --steps steps after --warmup, timed with device events.  With --trace (needs rocprofv3 on PATH) one more
run of each twin leg that was timed -- (c) in fp32, (e) per half type -- under `rocprofv3 --kernel-trace --stats`
gives, per precision, the share of this repository's kernels in the step's kernel time.  Appends one JSON line to
profiles/train/train_step.jsonl and prints it.  Not part of bench.py."""
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


def run_config(config, batch, steps, warmup, precision="fp32"):
    import torch
    from aind_exaspim_image_compression import inference
    from aind_exaspim_image_compression.machine_learning import losses, train, unet3d

    inference._miopen_defaults()
    torch.manual_seed(0)
    model = unet3d.UNet().cuda()
    net = model
    if config in "bd":
        model.to(memory_format=torch.channels_last_3d)
    if config in "ce":
        net = train.trainable_ndhwc(model, precision=precision)
        criterion = losses.SignalPreservingLoss()
    else:
        def criterion(pred, target, fg):          # the reference's expression, whatever the layout
            return ((1.0 + 20.0 * fg) * losses.charbonnier(pred - target, 1e-3)).mean()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    x = torch.randn(batch, 1, 64, 64, 64, device="cuda")
    y = x + 0.1 * torch.randn_like(x)
    fg = (torch.rand_like(x) < 0.1).float()
    scaler = torch.amp.GradScaler("cuda") if precision == "fp16" else None
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = train.train_step(net, opt, criterion, x, y, fg, scaler=scaler, precision=precision)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"config": config, "precision": precision, "ms": statistics.median(times), "loss": float(loss),
            "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30}


def child(args, config, prefix=(), precision="fp32"):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--config", config, "--batch", str(args.batch),
                          "--steps", str(args.steps), "--warmup", str(args.warmup), "--precision", precision]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    print(f"({config}) {precision}: {res['ms']:.1f} ms, peak {res['peak_gib']:.2f} GiB", file=sys.stderr, flush=True)
    return res


def kernel_shares(args, config, precision):
    """Per-kernel share (%) of this repository's kernels in the kernel time of the twin's leg: (c) in fp32, (e)
    under ``precision``."""
    with tempfile.TemporaryDirectory() as d:
        child(args, config, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"),
              precision=precision)
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
    ap.add_argument("--config", choices="abcde", help="run one configuration in this process (what the parent starts)")
    ap.add_argument("--precision", choices=["fp32", "fp16", "bf16", "all"], default="fp32",
                    help="fp32: legs (a), (b), (c); fp16 / bf16: legs (d), (e) under that autocast; all: the seven legs")
    ap.add_argument("--trace", action="store_true", help="also trace the kernels of the twin's legs, (c) / (e), with rocprofv3")
    args = ap.parse_args()
    if args.config:
        if (args.config in "abc") != (args.precision == "fp32"):
            ap.error("--config a, b, c run in fp32; d, e under --precision fp16 or bf16")
        print(json.dumps(run_config(args.config, args.batch, args.steps, args.warmup, args.precision)), flush=True)
        return
    line = {"batch": args.batch, "patch": 64, "dtype": args.precision, "steps": args.steps, "warmup": args.warmup}
    peak = {}
    if args.precision in ("fp32", "all"):
        res = {c: child(args, c) for c in "abc"}
        line.update({"ms_plain": res["a"]["ms"], "ms_plain_ndhwc": res["b"]["ms"], "ms_trainable_ndhwc": res["c"]["ms"]})
        peak.update({c: round(res[c]["peak_gib"], 2) for c in "abc"})
    for p in ("fp16", "bf16"):
        if args.precision in (p, "all"):
            res = {c: child(args, c, precision=p) for c in "de"}
            line.update({f"ms_autocast_ndhwc_{p}": res["d"]["ms"], f"ms_trainable_ndhwc_{p}": res["e"]["ms"]})
            peak.update({f"{c}_{p}": round(res[c]["peak_gib"], 2) for c in "de"})
    line["peak_gib"] = peak
    if args.trace:
        # the twin's leg of every precision that was timed: (c) for fp32, (e) for a half type
        legs = [("c", "fp32")] if args.precision in ("fp32", "all") else []
        legs += [("e", p) for p in ("fp16", "bf16") if args.precision in (p, "all")]
        line["own_kernel_share_percent"] = {p: kernel_shares(args, c, p) for c, p in legs}
    os.makedirs(os.path.join(ROOT, "profiles", "train"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train", "train_step.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
