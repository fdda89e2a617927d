#!/usr/bin/env python3
"""Benchmark of the BM4D denoise hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

Step  = one pass of the hot path over one synthetic uint16 volume that is already resident in
        HBM, all through the C-ABI (include/exabm4d.h):
        (1) exabm4d_denoise_u16_dev: uint16 counts -> fp32 - offset -> block matching ->
            hard-threshold stage -> basic estimate -> block matching -> Wiener stage -> normalise
            -> + offset -> clip -> rint -> uint16;
        (2) exabm4d_codec_encode_dev: the denoised volume coded losslessly in 64^3 chunks (EXAC v2:
            prediction from the voxel above / the plane before, 16 context tables per chunk,
            interleaved rANS; packed byte streams in HBM) -- the device counterpart of the
            reference's compute_cratio / write_zarr codec pass (utils/img_util.py:401-441,
            :935-950), whose codec is Blosc(zstd-5, SHUFFLE) (evaluate.py:40);
        (3) BASELINE config 5's lossy leg: exabm4d_dctq_forward_dev (8^3 block DCT, step Q_STEP)
            and exabm4d_codec_encode_dev on the int32 indices.
Metric = BASELINE.json's "denoised+encoded voxels/s on 1024^3 uint16".
N > 1 = one process per GPU (torch.distributed / RCCL for the barrier and the max over ranks);
        every rank denoises its own volume, no data-path collective ("weak" scaling).

One JSON line is printed by rank 0.  `roofline` is for the dominant kernel, timed live with HIP
events recorded on the stream the kernels run on (exabm4d "profile" option) inside the timed
region; its `traffic` and `valu` entries come from the committed rocprofv3 passes
(profiles/latest_counters.json names the profile and the commit) and are flagged stale when the
live kernel time has moved.  A plain run stops there: it sets up, warms up, times the steps, dumps
(--dump-outputs) and prints.  `--full` adds the legs below and `end_to_end`, after the timed region
and outside `value`.  `cpu_baseline` times the CPU port (oracle/exabm4d_cpu_port.c; the
reference's BM4D is a closed wheel that cannot travel) on this box's host cores: BASELINE configs
C1 and C2 fully, all usable cores and one thread, plus the host side of the encode half (the
reference's codec family: byte shuffle + zstd-5 per 64^3 chunk through libzstd).  `psnr` compares
the GPU's and the port's output on the same 256^3 volume against the clean volume.  `bm4dnet`
(config 3's learned stage, measured at the full 1024^3) and `encoded` (compression ratios of the
encode legs next to shuffle + zstd-5 on sampled chunks) are extra keys outside `value`.

`--dump-outputs DIR` (--mode volumes) writes what rank 0's last timed step computed as DIR/<name>.npy
(float32 / float64, under 64 MB in all): the denoised volume, the DCT indices and the two encode legs'
chunk sizes, offsets and packed streams -- all of an array when it is small, else a fixed seeded sample of
its elements in index order.  The input volume is a function of --size and the rank, so two builds run
with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "aind-exaspim-image-compression_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

Q_STEP = 8.0      # quantiser step of the timed config-5 leg (tools/rd_sweep.py sweeps it)
CHUNK = (64, 64, 64)  # reference compute_cratio patch_shape, utils/img_util.py:401
SIGMA = 24.0      # reference scripts/precompute.py:284
OFFSET = 37.0     # reference scripts/evaluate_bm4dnet.py:207
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec

# ALGORITHMIC bytes per input voxel of each kernel.  Match records are
# 16 x 4-byte keys per reference block = 64 B / 64 voxels = 1 B/voxel.
ALGO_BYTES_PER_VOXEL = {
    "counts_from_u16": 2 + 4,
    "blockmatch_ht": 2 + 1,          # stage-1 matching reads the uint16 planes (integer kernel)
    "stage_ht": 1 + 4 + 8,
    "normalize_basic": 8 + 4 + 2,    # ... + the estimate rounded to counts for stage 2's matching
    "blockmatch_wie": 2 + 1,         # the integer kernel again, on those counts
    "stage_wie": 1 + 4 + 4 + 8,
    "normalize_out": 8 + 2,
    # encode legs: volume / indices read once + the packed streams written (measured per run)
    "encode_u16": 2,
    "dct_quantise": 2 + 4,
    "encode_idx": 4,
}


_BRICK = {}


def _brick(seed):
    """128^3 structure brick: blurred bright random-walk 'neurites' (counts above pedestal)."""
    if seed not in _BRICK:
        from scipy.ndimage import gaussian_filter
        rng = np.random.default_rng([seed, 0xB41C])
        b = 128
        brick = np.zeros((b, b, b), dtype=np.float32)
        for _ in range(48):
            p = rng.uniform(0, b, 3)
            amp = float(np.exp(rng.uniform(np.log(100.0), np.log(8000.0))))
            for _ in range(int(rng.integers(200, 800))):
                p = np.clip(p + rng.normal(0, 0.7, 3), 0, b - 1)
                brick[int(p[0]), int(p[1]), int(p[2])] += amp
        _BRICK[seed] = gaussian_filter(brick, 1.5) * 12.0
    return _BRICK[seed]


def synth_u16(shape, seed, z_range=None):
    """Pedestal 37 + the mirror-tiled structure brick + N(0, 24) noise, rint, clip, uint16
    (SURVEY.md section 8d).  Deterministic and random-access in z: the noise of every 32-plane
    slab has its own seed, so a rank can regenerate exactly the planes [z0, z1) it holds.
    Slabs are made on host threads (numpy's generators and ufuncs release the GIL), a few planes
    at a time in reused buffers; a slab's generator is drawn from in plane order, so every voxel
    gets the value one whole-slab draw would give it."""
    brick = _brick(seed)
    b = brick.shape[0]
    nz, ny, nx = shape
    z0, z1 = (0, nz) if z_range is None else z_range

    def tile_axis(idx):
        idx = np.asarray(idx) % (2 * b)
        return np.where(idx < b, idx, 2 * b - 1 - idx)

    iy, ix = tile_axis(np.arange(ny)), tile_axis(np.arange(nx))
    out = np.empty((z1 - z0, ny, nx), dtype=np.uint16)
    slab = 32
    part = max(1, min(slab, (1 << 22) // max(1, ny * nx)))     # planes per piece: about 4 M voxels

    def fill(s0):
        rng = np.random.default_rng([seed, s0 // slab])
        a, e = max(z0, s0), min(z1, s0 + slab, nz)
        noise = np.empty((part, ny, nx), dtype=np.float32)
        clean = np.empty_like(noise)
        for p0 in range(s0, e, part):
            p1 = min(p0 + part, e)
            nb, cb = noise[:p1 - p0], clean[:p1 - p0]
            rng.standard_normal(dtype=np.float32, out=nb)      # planes below `a` are drawn and dropped
            if p1 <= a:
                continue
            np.take(brick[tile_axis(np.arange(p0, p1))][:, iy], ix, axis=2, out=cb)
            cb += np.float32(OFFSET)
            nb *= np.float32(SIGMA)
            nb += cb
            np.clip(nb, 0, 65535, out=nb)
            np.rint(nb, out=nb)
            lo = max(a, p0)
            out[lo - z0:p1 - z0] = nb[lo - p0:]

    starts = range((z0 // slab) * slab, z1, slab)
    threads = min(16, host_cpu()[1], len(starts))
    if threads <= 1:
        for s0 in starts:
            fill(s0)
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(fill, starts))
    return out


def synth_clean(shape, seed):
    """The noise-free volume synth_u16 adds its noise to (fp32 counts)."""
    brick = _brick(seed)
    b = brick.shape[0]

    def tile_axis(n):
        idx = np.arange(n) % (2 * b)
        return np.where(idx < b, idx, 2 * b - 1 - idx)

    iz, iy, ix = (tile_axis(n) for n in shape)
    return brick[iz][:, iy][:, :, ix] + np.float32(OFFSET)


def psnr_db(a, ref, peak):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(ref, np.float64)) ** 2))
    return float("inf") if mse == 0.0 else 10.0 * np.log10(peak * peak / mse)


DUMP_LIMIT = 64 << 20     # bytes of all --dump-outputs files together
DUMP_SEED = 0xD0D0


def dump_sample(a, k, tag, dtype):
    """a flattened, as `dtype`; when it holds more than k elements, a fixed seeded sample of k of them
    (index order; the sample depends on the element count and `tag` only)."""
    a = a.ravel()
    if a.size > k:
        rng = np.random.default_rng([DUMP_SEED, tag])
        a = a[np.sort(rng.choice(a.size, size=k, replace=False))]
    return a.astype(dtype)


def timed_outputs(denoised, indices=None, *encodes):
    """--dump-outputs of the volumes mode: the denoised uint16 volume (host array); `indices` = (count,
    device buffer) of the DCT leg's int32 indices; `encodes` = (name, chunks, streams, offsets, sizes)
    device buffers of each encode leg, as exabm4d_codec_encode_dev filled them."""
    out = {"denoised": dump_sample(denoised, 1 << 22, 0, np.float32)}
    if indices is not None:
        n, buf = indices
        out["dct_indices"] = dump_sample(buf.download((n,), np.int32), 1 << 21, 1, np.float64)
    for tag, (name, n, d_enc, d_off, d_sz) in enumerate(encodes, 2):
        off = d_off.download((n + 1,), np.uint64)
        out[f"{name}_sizes"] = d_sz.download((n,), np.uint32).astype(np.float64)
        out[f"{name}_offsets"] = off.astype(np.float64)
        out[f"{name}_stream"] = dump_sample(d_enc.download((int(off[-1]),), np.uint8), 1 << 20, tag, np.float32)
    return out


def write_outputs(path, arrays):
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit(f"--dump-outputs: {total} bytes is over the {DUMP_LIMIT}-byte limit")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), a)


def profile_record(kernel, shape, live_ms):
    """What the committed rocprofv3 passes say about `kernel` at this volume shape
    (profiles/latest_counters.json, written by tools/pmc_summary.py from SEPARATE --pmc passes of
    this same bench command; it names the profile directory and the commit that was profiled):
    HBM bytes per launch (FETCH_SIZE / WRITE_SIZE with the gfx950 correction) and the VALU counters.
    A record whose kernel time differs from the live one by more than 10 % is flagged stale."""
    try:
        with open(os.path.join(ROOT, "profiles", "latest_counters.json")) as f:
            t = json.load(f)
        if list(t["volume"]) != list(shape):
            return None
        rec = dict(t["kernels"][kernel])
    except (OSError, ValueError, KeyError):
        return None
    rec["source"] = {"file": t.get("source"), "commit": t.get("commit")}
    if rec.get("avg_ms"):
        rec["stale"] = bool(abs(live_ms - rec["avg_ms"]) > 0.1 * rec["avg_ms"])
    return rec


def host_cpu():
    """CPU model and the number of cores this process may actually use (affinity mask and cgroup
    quota -- a GPU box hands a job a share of its cores, omp_get_max_threads still sees them all)."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    usable = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            usable = max(1, min(usable, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return model, usable, os.cpu_count()


def cpu_baseline(seed, budget_s=30.0):
    """The CPU port (oracle/exabm4d_cpu_port.c: the specification of DESIGN.md 3 written for a
    many-core host -- shared cell sums, SIMD over the dx candidates and the transform lines,
    coloured parallel scatter; match tables bit-identical to the checker) on this box's host cores.
    BASELINE.md section 3: configs C1 (64^3) and C2 (256^3) timed fully, all usable cores and one
    thread (the 1-thread C2 leg is a 128^3 sample when the budget does not allow the full volume)."""
    from oracle import bm4d_oracle as O
    O.build()
    model, usable, visible = host_cpu()

    kept = {}

    def timed(edge, threads, reps=1):
        vol = synth_u16((edge,) * 3, seed)
        O.set_threads(threads)
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = O.bm4d_u16(vol, SIGMA, OFFSET, stages=2, port=True)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        kept[(edge, threads)] = out
        return {"edge": edge, "threads": threads, "seconds": round(best, 3),
                "voxels_per_s": vol.size / best}

    t_start = time.perf_counter()
    c1_all = timed(64, usable, reps=3)
    c1_one = timed(64, 1)
    c2_all = timed(256, usable)
    est_one = c2_all["seconds"] * usable * 0.8            # optimistic guess of the 1-thread C2 time
    left = budget_s - (time.perf_counter() - t_start)
    c2_one = timed(256, 1) if est_one < left else timed(128, 1)
    O.set_threads(usable)
    port256 = kept[(256, usable)]
    return port256, {
        "value": c2_all["voxels_per_s"],
        "unit": "voxels/s",
        "cores": usable,
        "kind": "port",
        "sample": f"256^3 uint16 synthetic volume (BASELINE config 2 size), two-stage BM4D, timed "
                  f"fully: {c2_all['seconds']} s on {usable} threads",
        "cpu_model": model,
        "cpus_visible": visible,
        # what the job may use of the box: quote the GPU / CPU ratio as "vs `cores` threads of the PORT", a
        # whole-box run of the port would be several times faster
        "share_of_box": round(usable / max(visible, 1), 4),
        "share_note": f"{usable} of {visible} visible CPUs are usable by this job (cgroup / affinity); "
                      "GPU / CPU ratios are against these threads of the port, never the reference",
        "c1_64_all_threads": c1_all,
        "c1_64_one_thread": c1_one,
        "c2_256_all_threads": c2_all,
        "one_thread_large": c2_one,
        "encode": cpu_encode_baseline(port256, usable),
    }


def end_to_end_leg(ctx, vol, d_in, d_out, params, stages):
    """host array -> host array for the bench volume, outside `value`.  (a) the three legs one
    after the other: H2D of the uint16 input, the denoise call, D2H of the uint16 output (pageable host
    arrays, as numpy hands them over; the destination is touched beforehand so that page faults are not
    timed); (b) the overlapped form a host caller would use for a volume of this size,
    exabm4d_denoise_chunked_u16_host (256^3 cores + 8-voxel halo, BASELINE config 4's chunk-local semantics:
    layers of chunks go up and come down while the neighbouring layer is in the kernels)."""
    import ctypes
    from aind_exaspim_image_compression import _native
    lib = _native.lib()
    out = np.empty(vol.shape, dtype=np.uint16)
    out.fill(1)                                            # touched: np.zeros would leave the page faults to the copy
    shape, n = vol.shape, vol.size
    ctx.sync()
    t0 = time.perf_counter()
    d_in.upload(vol)                                       # exabm4d_memcpy_h2d synchronises
    t1 = time.perf_counter()
    ctx.denoise_u16(d_in, d_out, shape, SIGMA, OFFSET, params=params, stages=stages)
    ctx.sync()
    t2 = time.perf_counter()
    ctx._check(lib.exabm4d_memcpy_d2h(ctx.handle, out.ctypes.data_as(ctypes.c_void_p), d_out.ptr, out.nbytes))
    t3 = time.perf_counter()
    res = {
        "volume": list(shape),
        "h2d_ms": 1e3 * (t1 - t0), "denoise_ms": 1e3 * (t2 - t1), "d2h_ms": 1e3 * (t3 - t2),
        "sequential_ms": 1e3 * (t3 - t0), "sequential_voxels_per_s": n / (t3 - t0),
        "h2d_GBs": vol.nbytes / (t1 - t0) / 1e9, "d2h_GBs": out.nbytes / (t3 - t2) / 1e9,
        "host_memory": "pageable numpy arrays",
        "note": "PCIe-inclusive, never the bench `value`; denoise only (the encode legs' output stays in HBM)",
    }
    try:
        out2 = np.empty(vol.shape, dtype=np.uint16)
        out2.fill(1)
        t0 = time.perf_counter()
        ctx.denoise_chunked_u16_host(vol, out2, SIGMA, OFFSET, chunk=256, halo=8, params=params, stages=stages)
        dt = time.perf_counter() - t0
        res["streamed_chunk_local"] = {
            "ms": 1e3 * dt, "voxels_per_s": n / dt,
            "what": "exabm4d_denoise_chunked_u16_host: 256^3 cores + 8 halo, uploads / downloads of the "
                    "neighbouring chunk layers under the kernels (1.2 x the voxels of the whole-volume call)",
        }
    except Exception as e:                               # the metric line must not die with the extra leg
        res["streamed_chunk_local"] = {"error": repr(e)}
    return res


def cpu_encode_baseline(den, threads):
    """Host side of the metric's encode half on the port's denoised 256^3 volume: the reference's
    loop (compute_cratio, utils/img_util.py:401-441) with its codec family -- byte shuffle + zstd
    level 5 per 64^3 chunk (Blosc(zstd, 5, SHUFFLE), evaluate.py:40) through libzstd via ctypes,
    chunks spread over `threads` host threads -- and this repo's coder restated in scalar C
    (oracle/exac_codec.c, one thread)."""
    from oracle import codec_oracle as co
    from oracle import zstd_ref
    res = {"sample": "the CPU port's denoised 256^3 uint16 volume, 64 chunks of 64^3"}
    if zstd_ref.available():
        zstd_ref.volume_size(den[:64], CHUNK, 5, threads)                # warm-up
        t0 = time.perf_counter()
        zbytes = zstd_ref.volume_size(den, CHUNK, 5, threads)
        dt = time.perf_counter() - t0
        res["shuffle_zstd5"] = {"codec": f"byte shuffle + zstd level 5 (libzstd {zstd_ref.version()}, ctypes), "
                                         "one frame per 64^3 chunk", "threads": threads,
                                "seconds": round(dt, 3), "voxels_per_s": den.size / dt,
                                "cratio": round(den.nbytes / zbytes, 3)}
    else:
        res["shuffle_zstd5"] = None
    t0 = time.perf_counter()
    ebytes = sum(len(co.encode(c)) for c in co.chunks(den, CHUNK))
    dt = time.perf_counter() - t0
    res["exac_v2_port"] = {"codec": "EXAC v2, scalar C restatement (oracle/exac_codec.c)", "threads": 1,
                           "seconds": round(dt, 3), "voxels_per_s": den.size / dt,
                           "cratio": round(den.nbytes / ebytes, 3)}
    return res


def bm4dnet_leg(vol, tune_edge=0):
    """BASELINE config 3's learned stage: device-resident predict() of the BM4DNet U-Net (PyTorch-ROCm /
    MIOpen only, per north_star; random-init weights -- throughput, not quality) on the bench volume
    itself: ONE timed call at the full size after a one-batch call that loads MIOpen's kernels.  Round 4:
    predict's default IS the fast path (NDHWC copy of the model + the find-db records shipped with the
    package + FAST find mode: inference._miopen_defaults); nothing is searched, on a fresh machine either.
    `cold_start` = what a fresh process pays before its first batch returns (the one-batch call).
    `reference_like` = the same call with fast=False and MIOpen left alone (EXABM4D_MIOPEN_DEFAULTS=0), in a
    child process of its own, on a `tune_edge`^3 sub-volume when tune_edge > 0 (rounds 1-3's default)."""
    import torch
    from aind_exaspim_image_compression import inference
    from aind_exaspim_image_compression.machine_learning import transforms as T
    from aind_exaspim_image_compression.machine_learning import unet3d
    torch.manual_seed(0)
    model = unet3d.UNet().cuda().eval()
    tf = T.build_transform({"kind": "offset",
                            "base": {"kind": "asinh", "params": {"offset": 0.0, "scale": 32.0}},
                            "params": {"offset": OFFSET}})
    edge = vol.shape[0]
    t0 = time.perf_counter()
    inference.predict(vol[:64, :220, :428], model, tf, batch_size=32, verbose=False)   # 1 x 4 x 8 patches: one full batch
    warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = inference.predict(vol, model, tf, batch_size=32, verbose=False)
    dt = time.perf_counter() - t0
    npatch = inference.count_patches(inference._ShapeOnly((1, 1) + vol.shape), 64, 12)
    # the forward passes alone (same NDHWC copy, same batch shape): what is left is transform, gather,
    # accumulate, finalise and the two host copies
    shadow = inference._ndhwc_shadow(model)
    x = torch.randn(32, 1, 64, 64, 64, device="cuda")
    with torch.no_grad():
        shadow(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            shadow(x)
        torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t1) / 5 * 1e3
    nbatch = -(-npatch // 32)
    res = {
        "what": f"inference.predict on the {edge}^3 uint16 bench volume: asinh transform, {npatch} patches "
                "of 64^3 (overlap 12, trim 5), batch 32, fp32 U-Net (12.9 M parameters, random init) through "
                "an NDHWC copy with MIOpen's tuned implicit-GEMM solvers (shipped find-db records, FAST find "
                "mode) whose GroupNorm + LeakyReLU pairs, max-pools and up-samplings are libexabm4d's NDHWC "
                "kernels, stitching and inverse transform on device, host to host, one timed call",
        "seconds": round(dt, 3),
        "cold_start_seconds": round(warm, 3),
        "voxels_per_s": vol.size / dt,
        "unet_tflops": npatch * 109.639e9 / dt / 1e12,
        "forward_ms_per_batch": round(fwd_ms, 2),
        "forward_tflops": 32 * 109.639e9 / (fwd_ms * 1e-3) / 1e12,
        "seconds_outside_the_forward_passes": round(dt - nbatch * fwd_ms * 1e-3, 3),
        "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE"),
        "miopen_user_db": os.environ.get("MIOPEN_USER_DB_PATH"),
        "extrapolation": ("measured at 1024^3" if npatch == 8000 else
                          f"measured at {edge}^3 ({npatch} patches); 1024^3 has 8000"),
        "low_edge_quirk_ok": bool(np.all(out[:5] == int(OFFSET))),      # inference.py:91-103
    }
    del out, shadow, x
    if tune_edge:
        res["reference_like"] = bm4dnet_reference_like(tune_edge)
    return res


def bm4dnet_reference_like(edge):
    """predict(..., fast=False) with MIOpen's own defaults in a fresh child process (the environment of
    rounds 1-3: default find mode, default layout) on an edge^3 volume: first-batch cost and steady rate."""
    code = (
        "import os, sys, time, json\n"
        "os.environ['EXABM4D_MIOPEN_DEFAULTS'] = '0'\n"
        f"sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'aind-exaspim-image-compression_amd')!r}]\n"
        "import numpy as np, torch, bench\n"
        "from aind_exaspim_image_compression import inference\n"
        "from aind_exaspim_image_compression.machine_learning import transforms as T, unet3d\n"
        "torch.manual_seed(0)\n"
        "model = unet3d.UNet().cuda().eval()\n"
        "tf = T.build_transform({'kind': 'offset', 'base': {'kind': 'asinh', 'params': {'offset': 0.0, 'scale': 32.0}}, 'params': {'offset': bench.OFFSET}})\n"
        f"vol = bench.synth_u16(({edge},) * 3, seed=1000)\n"
        "t0 = time.perf_counter(); inference.predict(vol[:116, :220, :220], model, tf, batch_size=32, verbose=False, fast=False); warm = time.perf_counter() - t0\n"   # 2 x 4 x 4 patches: one full batch
        "t0 = time.perf_counter(); inference.predict(vol, model, tf, batch_size=32, verbose=False, fast=False); dt = time.perf_counter() - t0\n"
        "n = inference.count_patches(inference._ShapeOnly((1, 1) + vol.shape), 64, 12)\n"
        "print(json.dumps({'edge': vol.shape[0], 'patches': n, 'cold_start_seconds': round(warm, 3), 'seconds': round(dt, 3), 'unet_tflops': n * 109.639e9 / dt / 1e12}))\n"
    )
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIOPEN_")}
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        return json.loads(line[-1]) if line else {"error": r.stderr[-400:]}
    except Exception as e:
        return {"error": repr(e)}


def zstd_comparison(den, raw, shape, sz_den, sz_raw, want=256):
    """The codec family the reference ships -- byte shuffle + zstd-5 per 64^3 chunk, libzstd through
    ctypes (oracle/zstd_ref.py) -- on a sample of the SAME chunks the device coder just coded
    (every k-th chunk in raster order, about `want` of them), outside the timed region."""
    from oracle import zstd_ref
    if not zstd_ref.available():
        return {"cratio_zstd5_shuffle": None}
    grid = [-(-n // c) for n, c in zip(shape, CHUNK)]
    nchunks = int(np.prod(grid))
    pick = list(range(0, nchunks, max(1, nchunks // want)))

    def box(c):
        z, y, x = c // (grid[1] * grid[2]), (c // grid[2]) % grid[1], c % grid[2]
        return (slice(64 * z, 64 * z + 64), slice(64 * y, 64 * y + 64), slice(64 * x, 64 * x + 64))

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, host_cpu()[1])) as ex:
        zd = list(ex.map(lambda c: zstd_ref.shuffle_zstd_size(den[box(c)], 5), pick))
        zr = list(ex.map(lambda c: zstd_ref.shuffle_zstd_size(raw[box(c)], 5), pick))
    rawb = float(sum(den[box(c)].nbytes for c in pick))
    return {
        "cratio_zstd5_shuffle": round(rawb / float(sum(zd)), 2),
        "cratio_zstd5_shuffle_raw": round(rawb / float(sum(zr)), 2),
        "cratio_denoised_same_chunks": round(rawb / float(sz_den[pick].sum()), 2),
        "cratio_raw_same_chunks": round(rawb / float(sz_raw[pick].sum()), 2),
        "zstd_sample": f"{len(pick)} of {nchunks} chunks (every {max(1, nchunks // want)}th in raster order), "
                       f"libzstd {zstd_ref.version()} level 5 on the byte-shuffled chunk, one frame per chunk",
    }


def torch_encode_legs(ctx, own, dev):
    """The metric's encode legs on a rank's own planes held in a torch tensor (slab / chunk modes):
    lossless EXAC of the uint16 planes, 8^3 DCT quantiser, EXAC of the indices; everything stays in
    HBM.  Returns (encode(out), sizes of the lossless chunks)."""
    import torch
    from aind_exaspim_image_compression import _native
    nchunks = int(np.prod([-(-m // c) for m, c in zip(own, CHUNK)]))
    cap16 = _native.codec_volume_bound(2, own, CHUNK)
    enc16 = torch.empty(cap16, dtype=torch.uint8, device=dev)
    off16 = torch.empty(nchunks + 1, dtype=torch.int64, device=dev)
    sz16 = torch.empty(nchunks, dtype=torch.int32, device=dev)
    nblk = int(np.prod([-(-m // 8) for m in own]))
    idx_shape, idx_chunk = (nblk, 8, 64), (512, 8, 64)
    nchunks_i = -(-nblk // 512)
    cap32 = _native.codec_volume_bound(4, idx_shape, idx_chunk)
    idx = torch.empty(nblk * 512, dtype=torch.int32, device=dev)
    enc32 = torch.empty(cap32, dtype=torch.uint8, device=dev)
    off32 = torch.empty(nchunks_i + 1, dtype=torch.int64, device=dev)
    sz32 = torch.empty(nchunks_i, dtype=torch.int32, device=dev)

    def encode(out):
        # `out` was produced on torch's current stream (a torch.cat / .contiguous() copy is
        # asynchronous): the coder runs on that stream too, not on the context's private one
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ctx.codec_encode(out, 2, own, CHUNK, out=enc16, out_capacity=cap16, offsets=off16,
                         sizes=sz16, totals=False)
        ctx.dctq_forward(out, own, Q_STEP, idx)
        ctx.codec_encode(idx, 4, idx_shape, idx_chunk, out=enc32, out_capacity=cap32,
                         offsets=off32, sizes=sz32, totals=False)
        ctx.sync()
        ctx.reset_stream()

    return encode, sz16


def run_slabs(args, rank, local_rank, world, dist, group=None):
    """N ranks, ONE volume of N*size planes: every rank holds its z-slab plus a 24-plane halo,
    runs stage 1 (uint16 matching), exchanges the basic estimate's halo with its slab neighbours
    (RCCL isend / irecv; 24 planes = 100 MB per neighbour at 1024^2, ~2 ms over xGMI against a
    ~0.7 s step, so it is not overlapped), runs stage 2, and quantises + encodes its own planes
    like the single-GPU step.  Weak scaling (size^3 voxels per rank)."""
    import torch
    from aind_exaspim_image_compression.distributed import (SlabDenoiser, denoise_slab_u16,
                                                            plan_slabs)
    n = args.size
    shape = (n * world, n, n)
    plan = plan_slabs(shape[0], world, rank)
    dev = torch.device("cuda", local_rank)
    host = synth_u16(shape, seed=2000, z_range=(plan.p0, plan.p1))
    raw = torch.from_numpy(host.view(np.int16)).to(dev)
    den = SlabDenoiser(host.shape, SIGMA, dev)
    ctx = den.ctx
    apply_env_options(ctx)
    own = (plan.z1 - plan.z0, n, n)
    encode, sz16 = torch_encode_legs(ctx, own, dev)

    def step():
        out = denoise_slab_u16(raw, plan, OFFSET, den, dist=dist, group=group).contiguous()
        if not args.no_encode:
            encode(out)
        return out

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier(group=group)
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if group is None else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        elapsed = float(t.item())
    if rank == 0:
        resid = (out[::8, ::8, ::8].to(torch.int32) & 0xFFFF).float() - \
                (raw[plan.core][::8, ::8, ::8].to(torch.int32) & 0xFFFF).float()
        emit(json.dumps({
            "metric": "denoised+encoded voxels/s on 1024^3 uint16",
            "value": world * n ** 3 * args.steps / elapsed,
            "unit": "voxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{shape[0]}x{n}x{n} uint16 volume in {world} z-slab(s), "
                                   "two-stage BM4D, 24-plane halo exchange of the basic estimate, "
                                   + ("no encode" if args.no_encode else
                                      f"then lossless + DCT q={Q_STEP} encode of the own planes"),
                       "volume": list(shape), "stages": 2,
                       "sharding": "z-slabs, RCCL point-to-point halo exchange"},
            "residual_std": float(resid.std()),
            "rank0_lossless_cratio": None if args.no_encode else
            round(2.0 * float(np.prod(own)) / float(sz16.sum().item()), 2),
        }))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_chunks(args, rank, local_rank, world, dist, group=None):
    """BASELINE config 4: N ranks, ONE volume of N*size planes in chunk-local mode -- 256^3 cores
    with an 8-voxel halo, every padded chunk denoised in isolation.  A rank owns whole layers of
    chunks; the only exchange is the raw uint16 input halo (8 planes to each slab neighbour, RCCL
    isend / irecv), overlapped with the chunk layers that do not need it.  Weak scaling."""
    import torch
    from aind_exaspim_image_compression.distributed import (ChunkedSlabDenoiser, denoise_chunked_slab,
                                                            plan_chunk_slabs)
    chunk, halo = args.chunk, 8
    # per-rank planes x rows x columns: --size^3 unless --shape names them (BASELINE config 4's share of
    # one rank of eight is --shape 256,4096,4096: the whole tile is 2048 x 4096 x 4096)
    pz, py, px = (args.size,) * 3 if not args.shape else tuple(int(v) for v in args.shape.split(","))
    shape = (pz * world, py, px)
    plan = plan_chunk_slabs(shape[0], world, rank, chunk=chunk, halo=halo)
    dev = torch.device("cuda", local_rank)
    host = synth_u16(shape, seed=3000, z_range=(plan.z0, plan.z1))
    own = torch.from_numpy(host.view(np.int16)).to(dev)
    del host
    raw = torch.zeros((plan.p1 - plan.p0, py, px), dtype=torch.int16, device=dev)
    den = ChunkedSlabDenoiser(SIGMA, OFFSET, dev, chunk=chunk, halo=halo)
    apply_env_options(den.ctx)
    own_shape = (plan.z1 - plan.z0, py, px)
    encode, sz16 = torch_encode_legs(den.ctx, own_shape, dev)

    def step():
        raw[plan.core] = own                   # only the owned planes are known before the exchange
        out = denoise_chunked_slab(raw, plan, den.run, chunk=chunk, dist=dist, group=group).contiguous()
        if not args.no_encode:
            encode(out)
        return out

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier(group=group)
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if group is None else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        elapsed = float(t.item())
    if rank == 0:
        resid = (out[::8, ::8, ::8].to(torch.int32) & 0xFFFF).float() - \
                (own[::8, ::8, ::8].to(torch.int32) & 0xFFFF).float()
        emit(json.dumps({
            "metric": "denoised+encoded voxels/s on 1024^3 uint16",
            "value": world * pz * py * px * args.steps / elapsed,
            "unit": "voxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{shape[0]}x{py}x{px} uint16 volume, chunk-local two-stage BM4D: "
                                   f"{chunk}^3 cores + {halo}-voxel halo, {world} z-slab(s) of whole "
                                   "chunk layers, raw-input halo exchange overlapped with interior layers",
                       "volume": list(shape), "stages": 2,
                       "encode": "none" if args.no_encode else
                       f"lossless EXAC + 8^3 DCT q={Q_STEP:g} + EXAC of the indices, on the own planes",
                       "sharding": "chunk layers per rank, RCCL point-to-point exchange of 8 input planes"},
            "residual_std": float(resid.std()),
            "rank0_lossless_cratio": None if args.no_encode else
            round(2.0 * float(np.prod(own_shape)) / float(sz16.sum().item()), 2),
        }))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def native_encode_legs(ctx, own):
    """torch_encode_legs on DeviceBuffers (the torch-free sharded modes)."""
    from aind_exaspim_image_compression import _native
    nchunks = int(np.prod([-(-m // c) for m, c in zip(own, CHUNK)]))
    cap16 = _native.codec_volume_bound(2, own, CHUNK)
    enc16, off16, sz16 = ctx.alloc(cap16), ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    nblk = int(np.prod([-(-m // 8) for m in own]))
    idx_shape, idx_chunk = (nblk, 8, 64), (512, 8, 64)
    nchunks_i = -(-nblk // 512)
    cap32 = _native.codec_volume_bound(4, idx_shape, idx_chunk)
    idx = ctx.alloc(4 * nblk * 512)
    enc32, off32, sz32 = ctx.alloc(cap32), ctx.alloc(8 * (nchunks_i + 1)), ctx.alloc(4 * nchunks_i)

    def encode(out_ptr):
        ctx.codec_encode(out_ptr, 2, own, CHUNK, out=enc16, out_capacity=cap16, offsets=off16, sizes=sz16, totals=False)
        ctx.dctq_forward(out_ptr, own, Q_STEP, idx)
        ctx.codec_encode(idx, 4, idx_shape, idx_chunk, out=enc32, out_capacity=cap32, offsets=off32, sizes=sz32,
                         totals=False)

    return encode, lambda: sz16.download((nchunks,), np.uint32)


def run_sharded_native(args, rank, local_rank, world):
    """--mode slabs | chunks with --comm native: the same two sharded modes WITHOUT torch -- DeviceBuffers, the
    context's stream, the halo exchange through exabm4d_halo_exchange_dev (ncclGroupStart / ncclSend / ncclRecv /
    ncclGroupEnd behind the C-ABI, csrc/comm_rccl.hip), the timed region bracketed by exabm4d_comm_max_f64_host
    (an RCCL all-reduce + stream synchronisation: barrier and MAX in one).  north_star: "PyTorch-ROCm used only
    for the bm4dnet stage ... RCCL over xGMI only for halo exchange"."""
    assert "torch" not in sys.modules, "the native sharded modes must not import torch"
    from aind_exaspim_image_compression import _native
    from aind_exaspim_image_compression.distributed import (denoise_chunked_slab_native, denoise_slab_u16_native,
                                                            plan_chunk_slabs, plan_slabs, rendezvous_comm)
    ctx = _native.context(local_rank)
    apply_env_options(ctx)
    comm = rendezvous_comm(ctx, rank, world)
    chunked = args.mode == "chunks"
    chunk, halo = args.chunk, 8
    pz, py, px = (args.size,) * 3 if not (chunked and args.shape) else tuple(int(v) for v in args.shape.split(","))
    shape = (pz * world, py, px)
    plan = plan_chunk_slabs(shape[0], world, rank, chunk=chunk, halo=halo) if chunked else plan_slabs(shape[0], world, rank)
    pshape = (plan.p1 - plan.p0, py, px)
    plane = py * px
    core = plan.core
    own_shape = (plan.z1 - plan.z0, py, px)
    # chunks: only the owned planes are known before the exchange; slabs: every rank reads its padded range
    host = synth_u16(shape, seed=3000 if chunked else 2000, z_range=(plan.z0, plan.z1) if chunked else (plan.p0, plan.p1))
    d_raw = ctx.alloc(2 * pshape[0] * plane).zero()
    own_host = host if chunked else host[core]
    if chunked:
        ctx._check(_native.lib().exabm4d_memcpy_h2d(ctx.handle, d_raw.ptr + 2 * core.start * plane, host.ctypes.data,
                                                    host.nbytes))
    else:
        d_raw.upload(host)
    encode, sizes16 = native_encode_legs(ctx, own_shape)
    last = [None]

    def step():
        if last[0] is not None:
            last[0].free()
        if chunked:
            out = denoise_chunked_slab_native(ctx, comm, d_raw, plan, pshape, SIGMA, OFFSET, chunk=chunk, halo=halo)
            own_ptr = out.ptr
        else:
            out = denoise_slab_u16_native(ctx, comm, d_raw, plan, pshape, SIGMA, OFFSET)
            own_ptr = out.ptr + 2 * core.start * plane
        if not args.no_encode:
            encode(own_ptr)
        last[0] = out
        return own_ptr

    for _ in range(args.warmup):
        step()
    comm.max(0.0)                                         # barrier
    t0 = time.perf_counter()
    for _ in range(args.steps):
        own_ptr = step()
    ctx.sync()
    elapsed = comm.max(time.perf_counter() - t0)          # ... and the slowest rank's time
    if rank == 0:
        out = np.empty(own_shape, np.uint16)
        ctx._check(_native.lib().exabm4d_memcpy_d2h(ctx.handle, out.ctypes.data, own_ptr, out.nbytes))
        resid = out[::8, ::8, ::8].astype(np.float32) - own_host[::8, ::8, ::8].astype(np.float32)
        emit(json.dumps({
            "metric": "denoised+encoded voxels/s on 1024^3 uint16",
            "value": world * pz * py * px * args.steps / elapsed,
            "unit": "voxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": (f"{shape[0]}x{py}x{px} uint16 volume, chunk-local two-stage BM4D: {chunk}^3 cores + "
                                    f"{halo}-voxel halo, {world} z-slab(s) of whole chunk layers" if chunked else
                                    f"{shape[0]}x{py}x{px} uint16 volume in {world} z-slab(s), two-stage BM4D, 24-plane "
                                    "halo exchange of the basic estimate"),
                       "volume": list(shape), "stages": 2,
                       "encode": "none" if args.no_encode else
                       f"lossless EXAC + 8^3 DCT q={Q_STEP:g} + EXAC of the indices, on the own planes",
                       "sharding": "z-slabs; halo exchange = exabm4d_halo_exchange_dev (RCCL send / recv behind the "
                                   "C-ABI), rendezvous and barrier without torch",
                       "comm": "native"},
            "residual_std": float(resid.std()),
            "rank0_lossless_cratio": None if args.no_encode else
            round(2.0 * float(np.prod(own_shape)) / float(sizes16().astype(np.uint64).sum()), 2),
        }))
    comm.max(0.0)
    comm.close()


ENV_OPTIONS = {                      # A/B switches of tools/dbg: environment variable -> exabm4d_set_option name
    "EXABM4D_STAGE_CHUNKS": "stage_chunks",      # z chunks of the stage kernels
    "EXABM4D_STAGE_STRIP": "stage_strip",        # stage kernels: tile columns in strips of n tile rows
    "EXABM4D_STAGE_PAIRVOL": "stage_pairvol",    # Wiener gathers from the interleaved (noisy, basic) volume
    "EXABM4D_BM_CARRY": "bm_carry",              # block matching: carry between the tiles of a column
    "EXABM4D_BM_XCD_MODE": "bm_xcd_mode",        # block matching: workgroup order
    "EXABM4D_ZERO_OVERLAP": "zero_overlap",      # the sums' memsets under block matching (second stream) or in line
}


def apply_env_options(ctx):
    for var, name in ENV_OPTIONS.items():
        if os.environ.get(var):
            ctx.set_option(name, int(os.environ[var]))


_RESULT_FD = None
RENDEZVOUS_NOTE = []          # non-empty when a multi-rank run could not use RCCL for its barrier (volumes mode only)


def quiet_stdout():
    """Multi-rank runs: collective back-ends may print to stdout (gloo announces its peers there), and
    the driver parses stdout as ONE JSON line.  Everything written to fd 1 from here on goes to stderr;
    the result line goes to the original stdout through emit()."""
    global _RESULT_FD
    if _RESULT_FD is None:
        sys.stdout.flush()
        _RESULT_FD = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    if _RESULT_FD is None:
        print(line, flush=True)
    else:
        os.write(_RESULT_FD, (line + "\n").encode())


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: this process starts N ranks of itself -- one per
    GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, the rendezvous on
    127.0.0.1 -- waits for them and exits with the first non-zero status.  It runs before anything
    here has touched the GPU (no torch, no libexabm4d.so in the parent): children are fresh
    processes, the independent-worker shape of the reference's scripts/precompute.py:215-228."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:            # a dead rank leaves the others in a collective
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="cubic volume edge per GPU")
    ap.add_argument("--stages", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=256, help="core edge of --mode chunks")
    ap.add_argument("--shape", default="", help="--mode chunks: planes,rows,columns PER RANK instead of --size^3 "
                                                "(256,4096,4096 on 8 ranks is BASELINE config 4's tile)")
    ap.add_argument("--mode", choices=["volumes", "slabs", "chunks"], default="volumes",
                    help="N>1 sharding: 'volumes' = one independent volume per rank, no "
                         "data-path collective (default); 'slabs' = one (N*size) x size x size "
                         "volume split into z-slabs with an RCCL halo exchange of the basic "
                         "estimate between the two stages (distributed.py); 'chunks' = BASELINE "
                         "config 4: the same volume in chunk-local mode (--chunk^3 cores + 8-voxel "
                         "halo), raw-input halo exchange only")
    ap.add_argument("--comm", choices=["torch", "native"], default="torch",
                    help="--mode slabs | chunks: 'torch' = torch.distributed point-to-point (RCCL under the nccl "
                         "backend); 'native' = exabm4d_halo_exchange_dev, rendezvous and barrier without importing torch")
    ap.add_argument("--no-encode", action="store_true",
                    help="time the denoiser alone (the metric's step includes the encode legs)")
    ap.add_argument("--full", action="store_true",
                    help="--mode volumes: after the timed steps, also run the legs outside `value` -- `encoded` "
                         "(the coder on the noisy input, shuffle + zstd-5 on sampled chunks), and at N = 1 "
                         "`end_to_end`, `cpu_baseline` + `psnr` and `bm4dnet` (each can be switched off below); "
                         "without it the run does the timed steps and the result line only")
    ap.add_argument("--end-to-end", type=int, default=1,
                    help="with --full, 0: skip the host-to-host legs (H2D + denoise + D2H, and the streamed "
                         "chunk-local call) reported next to `value` at N = 1")
    ap.add_argument("--cpu-sample", type=int, default=1,
                    help="with --full, 0 disables the CPU-baseline leg (C1 64^3 and C2 256^3 timed fully on the "
                         "host) and the PSNR comparison")
    ap.add_argument("--bm4dnet", type=int, default=1,
                    help="with --full: BASELINE config 3's learned stage, predict() of the BM4DNet U-Net on the "
                         "bench volume itself (1024^3 by default: ~18 s), reported as extra keys; 0 disables")
    ap.add_argument("--bm4dnet-tune", type=int, default=256,
                    help="with --full: edge of the volume the reference-like path (fast=False, MIOpen's own "
                         "defaults, a fresh child process: ~20 s of solver selection) is measured on; 0 disables")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="--mode volumes: write what rank 0's last timed step computed to DIR/<name>.npy "
                         "(float32 / float64, seeded samples of the large arrays, under 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.mode != "volumes":
        ap.error("--dump-outputs needs --mode volumes")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))     # every mode: volumes, slabs, chunks

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    if os.environ.get("BENCH_FAIL_RANK") == str(rank) and world > 1:
        raise SystemExit(3)                     # tests: a rank that dies must fail the launcher

    if args.comm == "native" and args.mode in ("slabs", "chunks"):
        if os.environ.get("BENCH_REHEARSAL"):
            local_rank = 0                      # a one-GPU box can rehearse world = 1 only (RCCL: one rank per device)
        if world > 1:
            quiet_stdout()
        return run_sharded_native(args, rank, local_rank, world)

    dist = None
    torch = None
    group = None
    # BENCH_REHEARSAL=1: rehearse the multi-rank control flow on a box with ONE GPU -- gloo
    # rendezvous, every rank on device 0 (never the measured configuration).
    rehearsal = os.environ.get("BENCH_REHEARSAL") == "1"
    if world > 1:
        quiet_stdout()
        import datetime
        import torch
        import torch.distributed as dist
        # The ranks ALWAYS meet over gloo first; RCCL comes up as a second group and the ranks AGREE (one MIN
        # all-reduce over gloo) whether it did.  A rank that alone falls back would leave the others inside an
        # RCCL collective until its timeout.
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
        if rehearsal:
            local_rank = 0
        else:
            if os.environ.get("BENCH_REHEARSAL") == "2":     # tests: the RCCL rendezvous fails, on a one-GPU box
                local_rank = 0
            torch.cuda.set_device(local_rank)
            ok, why = 1, ""
            try:
                if os.environ.get("BENCH_REHEARSAL") == "2":
                    raise RuntimeError("rehearsal: RCCL forced down")
                group = dist.new_group(backend="nccl", timeout=datetime.timedelta(seconds=180))
                probe = torch.ones(1, device=torch.device("cuda", local_rank))
                dist.all_reduce(probe, group=group)          # builds the RCCL communicator now, not inside the timed region
                torch.cuda.synchronize()
                assert int(probe.item()) == world
            except Exception as exc:                         # noqa: BLE001
                ok, why = 0, repr(exc)
                print(f"[bench] rank {rank}: RCCL did not come up ({exc!r})", file=sys.stderr, flush=True)
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)      # over gloo: every rank learns the common answer
            if int(flag.item()) == 0:
                # The default mode has no data-path collective (one independent volume per rank): the rendezvous
                # only brackets the timed region, gloo does that as well and the line says so.  The slab / chunk
                # modes exchange device planes: they stop, all ranks together, with a non-zero status.
                group = None
                if args.mode != "volumes":
                    raise SystemExit(f"rank {rank}: RCCL is down on at least one rank ({why or 'another rank'}); "
                                     f"--mode {args.mode} needs it")
                RENDEZVOUS_NOTE.append("gloo (RCCL did not come up on every rank)")
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    # (import order of torch and libexabm4d.so is free: _native.lib() settles which HIP runtime the
    # process uses -- INTEGRATION.md 1d)
    from aind_exaspim_image_compression import _native

    if args.mode == "slabs":
        return run_slabs(args, rank, local_rank, world, dist, group)
    if args.mode == "chunks":
        return run_chunks(args, rank, local_rank, world, dist, group)

    ctx = _native.context(local_rank)
    shape = (args.size,) * 3
    nvox = int(np.prod(shape))
    vol = synth_u16(shape, seed=1000 + rank)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    params = _native.default_params()

    def barrier():
        ctx.sync()
        if dist is not None:
            torch.cuda.synchronize()
            dist.barrier(group=group)
            torch.cuda.synchronize()

    # encode legs: packed streams, offsets and sizes stay in HBM
    nchunks = int(np.prod([-(-n // c) for n, c in zip(shape, CHUNK)]))
    cap16 = _native.codec_volume_bound(2, shape, CHUNK)
    d_enc16, d_off16, d_sz16 = ctx.alloc(cap16), ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    nblk = int(np.prod([-(-n // 8) for n in shape]))
    idx_shape, idx_chunk = (nblk, 8, 64), (512, 8, 64)       # 2^18 consecutive indices per chunk
    nchunks_i = -(-nblk // 512)
    cap32 = _native.codec_volume_bound(4, idx_shape, idx_chunk)
    d_idx = ctx.alloc(4 * nblk * 512)
    d_enc32, d_off32, d_sz32 = ctx.alloc(cap32), ctx.alloc(8 * (nchunks_i + 1)), ctx.alloc(4 * nchunks_i)
    ev = [ctx.event() for _ in range(4)]

    def step():
        ctx.denoise_u16(d_in, d_out, shape, SIGMA, OFFSET, params=params, stages=args.stages)
        if args.no_encode:
            return
        ctx.record(ev[0])
        ctx.codec_encode(d_out, 2, shape, CHUNK, out=d_enc16, out_capacity=cap16, offsets=d_off16,
                         sizes=d_sz16, totals=False)
        ctx.record(ev[1])
        ctx.dctq_forward(d_out, shape, Q_STEP, d_idx)
        ctx.record(ev[2])
        ctx.codec_encode(d_idx, 4, idx_shape, idx_chunk, out=d_enc32, out_capacity=cap32,
                         offsets=d_off32, sizes=d_sz32, totals=False)
        ctx.record(ev[3])

    ctx.set_option("profile", 1)
    apply_env_options(ctx)
    for _ in range(args.warmup):
        step()
    barrier()
    phase_ms = {}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        for k, v in ctx.profile_read().items():      # waits for this step's events only
            phase_ms[k] = phase_ms.get(k, 0.0) + v
        if not args.no_encode:
            for i, k in enumerate(("encode_u16", "dct_quantise", "encode_idx")):
                phase_ms[k] = phase_ms.get(k, 0.0) + ctx.elapsed_ms(ev[i], ev[i + 1])
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if group is None else f"cuda:{local_rank}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        elapsed = float(t.item())

    # size-independent sanity property at full size: output is a denoised version of the input
    # (the first 64 planes, or the whole volume when a dump or the --full legs need it)
    whole = args.full or (args.dump_outputs and rank == 0)
    out = d_out.download(shape if whole else (min(64, shape[0]),) + shape[1:], np.uint16)
    sl = (slice(0, min(64, shape[0])),)
    resid = out[sl].astype(np.float32) - vol[sl].astype(np.float32)
    resid_std = float(resid.std())
    if args.dump_outputs and rank == 0:
        # the buffers still hold the last timed step's results (the end-to-end leg reuses d_out later)
        legs = () if args.no_encode else ((nblk * 512, d_idx), ("encode_u16", nchunks, d_enc16, d_off16, d_sz16),
                                          ("encode_idx", nchunks_i, d_enc32, d_off32, d_sz32))
        write_outputs(args.dump_outputs, timed_outputs(out, *legs))
    encoded = None
    if args.full and not args.no_encode:
        sz16 = d_sz16.download((nchunks,), np.uint32).astype(np.uint64)
        sz32 = d_sz32.download((nchunks_i,), np.uint32).astype(np.uint64)
        # the same coder on the noisy input, outside the timed region: the reference reports
        # cratio(raw) next to cratio(denoised) (scripts/evaluate_bm4dnet.py:141-145)
        d_szraw = ctx.alloc(4 * nchunks)
        raw_bytes, _ = ctx.codec_encode(d_in, 2, shape, CHUNK, sizes=d_szraw)
        szraw = d_szraw.download((nchunks,), np.uint32).astype(np.uint64)
        d_szraw.free()
        encoded = {
            "codec": "EXAC v2: up/back prediction, 64-symbol residual alphabet + raw bits, 16 context "
                     "tables per 64^3 chunk, 64 interleaved rANS states (DESIGN.md 3.11b)",
            "cratio_denoised": round(2.0 * nvox / float(sz16.sum()), 2),
            "cratio_raw": round(2.0 * nvox / float(raw_bytes), 2),
            "lossless_bytes": int(sz16.sum()),
            "dct_q": Q_STEP,
            "dct_bits_per_voxel": 8.0 * float(sz32.sum()) / nvox,
        }
        if rank == 0:
            encoded.update(zstd_comparison(out, vol, shape, sz16, szraw))

    if rank == 0:
        phase_avg = {k: v / max(args.steps, 1) for k, v in phase_ms.items() if v > 0}
        kern = {k: v for k, v in phase_avg.items() if k in ALGO_BYTES_PER_VOXEL}
        dom = max(kern, key=kern.get)
        achieved = ALGO_BYTES_PER_VOXEL[dom] * nvox / (kern[dom] * 1e-3) / 1e9
        rec = profile_record(dom, shape, kern[dom]) or {}
        roofline = {
            "bound": "hbm",
            "kernel": dom,
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": rec.get("hbm_bytes"),
            "traffic_source": rec.get("source"),
            "traffic_stale": rec.get("stale"),
            "algorithmic_bytes_per_voxel": ALGO_BYTES_PER_VOXEL[dom],
            "avg_ms": kern[dom],
        }
        if rec.get("valu_busy_cycles"):
            # the kernel is compute-bound: its honest ceiling is the vector ALU, not HBM.  Busy
            # cycles of the 1024 SIMDs (SQ_ACTIVE_INST_VALU, quad-cycles x 4) against the live
            # kernel time at the 2.4 GHz peak clock (the chip clocks lower under load, so this
            # fraction is a lower bound on the utilisation actually reached).
            simd_cycles = 1024 * 2.4e9 * kern[dom] * 1e-3
            roofline["valu"] = {
                "bound": "valu_issue",
                "insts_per_launch": rec.get("valu_insts"),
                "busy_cycles_per_launch": rec["valu_busy_cycles"],
                "peak_cycles": simd_cycles,
                "frac": rec["valu_busy_cycles"] / simd_cycles,
            }
        # every kernel of the step against both ceilings (same sources as above)
        every = {}
        for k, ms in sorted(kern.items(), key=lambda kv: -kv[1]):
            r = profile_record(k, shape, ms) or {}
            gbs = ALGO_BYTES_PER_VOXEL[k] * nvox / (ms * 1e-3) / 1e9
            every[k] = {"avg_ms": ms, "achieved_GBs": gbs, "hbm_frac": gbs / HBM_PEAK_GBS,
                        "traffic": r.get("hbm_bytes"),
                        "valu_frac": (r["valu_busy_cycles"] / (1024 * 2.4e9 * ms * 1e-3)
                                      if r.get("valu_busy_cycles") else None),
                        "stale": r.get("stale")}
        roofline["every_kernel"] = every
        result = {
            "metric": "denoised+encoded voxels/s on 1024^3 uint16",
            "value": world * nvox * args.steps / elapsed,
            "unit": "voxels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{args.size}^3 uint16 volume per GPU, two-stage BM4D "
                            "(hard-threshold + Wiener), 8^3 blocks step 4, 11^3 search, "
                            "16-block groups, sigma 24, offset 37; u16 in HBM -> u16 in HBM"
                            if args.stages == 2 else
                            f"{args.size}^3 uint16 volume per GPU, hard-threshold stage only",
                "volume": list(shape),
                "stages": args.stages,
                "encode": "none" if args.no_encode else
                          f"lossless EXAC of the denoised volume in 64^3 chunks + config-5 leg "
                          f"(8^3 block DCT, q = {Q_STEP:g}, EXAC of the int32 indices)",
                "sharding": "one independent volume per rank, no data-path collective",
                **({"rendezvous": RENDEZVOUS_NOTE[0]} if RENDEZVOUS_NOTE else {}),
            },
            "roofline": roofline,
            "phase_ms": phase_avg,
            "residual_std": resid_std,
        }
        if encoded is not None:
            result["encoded"] = encoded
        if args.full and args.end_to_end and world == 1:
            result["end_to_end"] = end_to_end_leg(ctx, vol, d_in, d_out, params, args.stages)
        if args.full and args.cpu_sample > 0 and world == 1:      # reported baseline: rank 0 at N = 1 only
            port256, result["cpu_baseline"] = cpu_baseline(seed=1000)
            # PSNR (BASELINE.json's metric names it): GPU and CPU port on the SAME 256^3 volume
            # against the clean volume the noise was added to; delta < 0.01 dB is the bar
            v256 = synth_u16((256,) * 3, seed=1000)
            b_in, b_out = ctx.to_device(v256), ctx.alloc(v256.nbytes)
            ctx.denoise_u16(b_in, b_out, v256.shape, SIGMA, OFFSET, params=params, stages=args.stages)
            gpu256 = b_out.download(v256.shape, np.uint16)
            # a second launch on the same input: the aggregation sums are integers, so the
            # arrival order of the atomics cannot show -- the same bytes, and the CPU port's
            ctx.denoise_u16(b_in, b_out, v256.shape, SIGMA, OFFSET, params=params, stages=args.stages)
            again256 = b_out.download(v256.shape, np.uint16)
            b_in.free()
            b_out.free()
            clean = synth_clean(v256.shape, 1000)
            peak = float(clean.max() - clean.min())
            d = np.abs(gpu256.astype(np.int32) - port256.astype(np.int32))
            result["psnr"] = {
                "volume": "256^3 bench-synthetic uint16 (BASELINE config 2 size), sigma 24",
                "peak": peak, "peak_is": "range of the clean volume (counts)",
                "noisy_vs_clean": psnr_db(v256, clean, peak),
                "gpu_vs_clean": psnr_db(gpu256, clean, peak),
                "cpu_vs_clean": psnr_db(port256, clean, peak),
                "delta_db": psnr_db(gpu256, clean, peak) - psnr_db(port256, clean, peak),
                # None = identical volumes (no finite PSNR); rounds 1-3: ~115 dB, up to 4 counts on rare voxels
                "gpu_vs_cpu": None if not d.any() else psnr_db(gpu256, port256, peak),
                "gpu_equals_cpu": bool(not d.any()),
                "second_launch_identical": bool(np.array_equal(gpu256, again256)),
                "max_abs_u16": int(d.max()), "frac_differing": float(np.mean(d > 0)),
                "frac_beyond_one_count": float(np.mean(d > 1)),
            }
        if args.full and args.bm4dnet > 0 and world == 1:
            # BASELINE config 3's learned stage, after the timed region and outside `value`
            for buf in (d_in, d_out, d_idx, d_enc16, d_enc32):
                buf.free()
            try:
                result["bm4dnet"] = bm4dnet_leg(vol, tune_edge=args.bm4dnet_tune)
            except Exception as e:                    # the metric line must not die with the extra leg
                result["bm4dnet"] = {"error": repr(e)}
        emit(json.dumps(result))

    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
