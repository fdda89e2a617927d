"""Throughput of the BM4DNet stage (PyTorch-ROCm U-Net inside the device-resident predict()), in fp32 and in
the reduced precisions of predict(precision=...).  Not part of bench.py's metric; reported in DESIGN.md for
BASELINE config 3."""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
from aind_exaspim_image_compression import inference  # noqa: E402
from aind_exaspim_image_compression.machine_learning import transforms as T  # noqa: E402
from aind_exaspim_image_compression.machine_learning import unet3d  # noqa: E402

TF_CFG = {"kind": "offset", "base": {"kind": "asinh", "params": {"offset": 0.0, "scale": 32.0}},
          "params": {"offset": 37.0}}


def precisions():
    """predict(precision=...) in a process of its own whose first convolution runs under predict's MIOpen defaults
    (shipped records, FAST mode): the NDHWC shadow's forward per batch of 32 x 64^3 and predict(256^3) per
    precision, and how far each half precision's counts are from fp32's."""
    inference._miopen_defaults()
    torch.manual_seed(0)
    model = unet3d.UNet().cuda().eval()
    x = torch.randn(32, 1, 64, 64, 64, device="cuda")
    tf = T.build_transform(TF_CFG)
    vol = np.random.default_rng(0).integers(0, 3000, size=(256, 256, 256)).astype(np.uint16)
    outs = {}
    for prec in ("fp32", "fp16", "bf16"):
        amp_dtype = inference.PRECISIONS[prec]
        shadow = inference._ndhwc_shadow(model, half=amp_dtype is not None)
        with torch.no_grad(), torch.autocast("cuda", dtype=amp_dtype or torch.float16, enabled=amp_dtype is not None):
            for _ in range(2):
                shadow(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                shadow(x)
            torch.cuda.synchronize()
            fwd = (time.perf_counter() - t0) / 5
        del shadow
        inference.predict(vol[:64, :64, :64], model, tf, verbose=False, precision=prec)
        t0 = time.perf_counter()
        outs[prec] = inference.predict(vol, model, tf, batch_size=32, verbose=False, precision=prec)
        dt = time.perf_counter() - t0
        line = (f"precision={prec}: forward, batch 32 x 64^3: {fwd*1e3:.1f} ms ({32*109.64e9/fwd/1e12:.1f} TFLOP/s); "
                f"predict(256^3): {dt:.2f} s = {vol.size/dt:.3e} voxels/s")
        if prec != "fp32":
            d = np.abs(outs[prec].astype(np.int64) - outs["fp32"].astype(np.int64))
            line += f"; |counts - fp32's|: mean {d.mean():.3g}, max {d.max()}"
        print(line, flush=True)


if sys.argv[1:] == ["--precisions"]:
    precisions()
    sys.exit(0)

torch.manual_seed(0)
model = unet3d.UNet().cuda().eval()
x = torch.randn(32, 1, 64, 64, 64, device="cuda")
for name, ctxm in (("fp32", torch.autocast("cuda", enabled=False)),
                   ("bf16 autocast", torch.autocast("cuda", dtype=torch.bfloat16)),
                   ("fp16 autocast", torch.autocast("cuda", dtype=torch.float16))):
    with torch.no_grad(), ctxm:
        for _ in range(2):
            model(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 3
        for _ in range(n):
            model(x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
    print(f"U-Net forward, batch 32 x 64^3, {name}: {dt*1e3:.1f} ms  "
          f"({32*109.64e9/dt/1e12:.1f} TFLOP/s, {32*54**3/dt:.3e} output voxels/s)", flush=True)

tf = T.build_transform(TF_CFG)
vol = np.random.default_rng(0).integers(0, 3000, size=(256, 256, 256)).astype(np.uint16)
inference.predict(vol[:64, :64, :64], model, tf, verbose=False)
t0 = time.perf_counter()
out = inference.predict(vol, model, tf, batch_size=32, verbose=False)
dt = time.perf_counter() - t0
print(f"predict(256^3, 125 patches, fp32): {dt:.2f} s = {vol.size/dt:.3e} voxels/s", flush=True)

ident = torch.nn.Identity().cuda()
t0 = time.perf_counter()
inference.predict(vol, ident, tf, batch_size=32, verbose=False)
dt = time.perf_counter() - t0
print(f"predict(256^3) stitching alone (identity model): {dt*1e3:.1f} ms", flush=True)

# opt-in MIOpen tuning (inference.tune_model): search cost and steady state
t0 = time.perf_counter()
inference.tune_model(model)
inference.predict(vol, model, tf, batch_size=32, verbose=False)
first = time.perf_counter() - t0
t0 = time.perf_counter()
inference.predict(vol, model, tf, batch_size=32, verbose=False)
dt = time.perf_counter() - t0
print(f"tune_model: first predict(256^3) {first:.1f} s (solver search), then {dt:.2f} s = "
      f"{vol.size/dt:.3e} voxels/s", flush=True)

# predict(precision=...) in a fresh process (this one's convolutions ran before predict's MIOpen defaults)
subprocess.run([sys.executable, os.path.abspath(__file__), "--precisions"], check=True)
