"""Error-bounded lossy store on the bench volume: for each bound delta, bits per voxel and ratio
of the bounded store next to the lossless store and to the best single ladder step that meets the same bound
everywhere (the existing DCT path: bench.py's index layout), the realised lmax, the share of lossless chunks and
the histogram of j*, and device milliseconds (HIP events) of the ladder kernel, the whole bounded encode, the
bounded decode and today's int32 decode + dctq_inverse at that global step.

    python tools/bounded_sweep.py [edge=1024] [deltas=1,2,4,8,16] [sigma=24] > bounded_sweep.json

With ``--granularity block`` the store with a step per 8^3 block is measured next to the per-chunk
one, both in the same session: bits per voxel, the shares of verbatim blocks and of mode-0 chunks, the histogram of the
block steps and what an order-0 code of the step plane would save, and device milliseconds of the select kernel, the
whole encode and the decode, each with its ratio to the per-chunk ladder kernel, encode and decode.  ``--fg-error 0,1``
adds the rows with that foreground bound for the bounds 4, 8 and 16 (``FG_DELTAS``); the foreground mask of the sweep is
``denoised > offset + 3 sigma`` (it is the sweep's own choice, stated in the output; callers bring their masks).

    python tools/bounded_sweep.py 1024 1,2,4,8,16 --granularity block --fg-error 0,1 \
        > profiles/bounded/block_bounded_sweep_1024.json

With ``--noise-k 0.25,0.5,1,2`` (block granularity) the bound comes from the data: a Poisson-Gaussian
volume is made, its parameters are re-estimated from it (``estimate_poisson_gaussian``), and for every k the store under
``bound_table(params, k)`` is measured next to the two constant bounds a user would otherwise choose between, the
table's value at the pedestal and at the 99.9th-percentile intensity: bits per voxel, mode-0 and verbatim shares, step
histogram, and device milliseconds of the select kernel with and without the table.

    python tools/bounded_sweep.py 1024 --granularity block --noise-k 0.25,0.5,1,2 \
        > profiles/bounded/noise_bounded_sweep_1024.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, ROOT)

from aind_exaspim_image_compression import _native  # noqa: E402
from aind_exaspim_image_compression.utils import dct_quant  # noqa: E402
from aind_exaspim_image_compression.utils.block_bounded_codec import plane_bytes  # noqa: E402
from aind_exaspim_image_compression.utils.bounded_codec import LADDER, STEPS, parse_header  # noqa: E402
import bench  # noqa: E402


def timed(ctx, fn, reps=3):
    """Device ms of fn() (median of reps, after one warm-up call that also sizes the scratch)."""
    return float(np.median(timed_all(ctx, fn, reps)))


def timed_all(ctx, fn, reps=3):
    """The reps device times themselves, for callers that state the spread."""
    fn()
    a, b = ctx.event(), ctx.event()
    out = []
    for _ in range(reps):
        ctx.record(a)
        fn()
        ctx.record(b)
        ctx.sync()
        out.append(ctx.elapsed_ms(a, b))
    return [float(t) for t in out]


def sweep(edge, deltas, sigma, seed=1000):
    shape, chunk = (edge,) * 3, bench.CHUNK
    n = edge ** 3
    ctx = _native.context(0)
    d_noisy, d_den, d_rec = ctx.to_device(bench.synth_u16(shape, seed)), ctx.alloc(2 * n), ctx.alloc(2 * n)
    ctx.denoise_u16(d_noisy, d_den, shape, sigma, bench.OFFSET)
    ctx.sync()
    d_noisy.free()
    grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
    nchunks = int(np.prod(grid))
    lossless, _ = ctx.codec_encode(d_den, 2, shape, chunk)
    d_err = ctx.alloc(4 * STEPS * nchunks)
    ladder_ms = timed(ctx, lambda: ctx.dctq_ladder_errors(d_den, shape, chunk, d_err))
    errs = d_err.download((nchunks, STEPS), np.uint32)
    cap = _native.bounded_volume_bound(shape, chunk)
    d_out, d_off, d_sz = ctx.alloc(cap), ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    nblk = int(np.prod([-(-s // 8) for s in shape]))
    d_idx = ctx.alloc(4 * 512 * nblk)
    icap = _native.codec_volume_bound(4, (nblk, 8, 64), dct_quant.INDEX_CHUNK)
    d_iout, d_ioff = ctx.alloc(icap), ctx.alloc(8 * (nblk // 512 + 2))
    rows = []
    for delta in deltas:
        enc_ms = timed(ctx, lambda: ctx.bounded_encode(d_den, shape, chunk, delta, out=d_out, out_capacity=cap,
                                                       offsets=d_off, sizes=d_sz, totals=False))
        coded, container = ctx.bounded_encode(d_den, shape, chunk, delta, out=d_out, out_capacity=cap,
                                              offsets=d_off, sizes=d_sz)
        dec_ms = timed(ctx, lambda: ctx.bounded_decode(d_out, container, d_off, shape, chunk, d_rec))
        err = ctx.masked_error_stats(d_rec, np.uint16, d_den, np.uint16, None, n)
        data = d_out.download((container,), np.uint8)
        offs = d_off.download((nchunks + 1,), np.uint64)
        steps = [parse_header(data[int(o):int(o) + 32].tobytes() + b"\0")["j"] for o in offs[:-1]]
        hist = np.bincount([j for j in steps if j is not None], minlength=STEPS)
        row = {"max_error": delta, "bits_per_voxel": 8.0 * coded / n, "cratio": 2.0 * n / coded,
               "coded_bytes": int(coded), "lmax": float(err[6]), "mae": float(err[1] / n),
               "lossless_chunk_share": sum(j is None for j in steps) / nchunks,
               "j_star_histogram": {f"{float(LADDER[j]):g}": int(hist[j]) for j in range(STEPS) if hist[j]},
               "device_ms_ladder_kernel": ladder_ms, "device_ms_bounded_encode": enc_ms,
               "device_ms_bounded_decode": dec_ms}
        ok = [j for j in range(STEPS) if np.all(errs[:, j] <= delta)]
        if ok:
            q = float(LADDER[max(ok)])
            rd = dct_quant.rate_distortion_device(ctx, d_den, shape, q, d_idx=d_idx, d_rec=d_rec)
            ctx.codec_encode(d_idx, 4, (nblk, 8, 64), dct_quant.INDEX_CHUNK, out=d_iout, out_capacity=icap,
                             offsets=d_ioff)
            _, icont = ctx.codec_encode(d_idx, 4, (nblk, 8, 64), dct_quant.INDEX_CHUNK, out=d_iout,
                                        out_capacity=icap, offsets=d_ioff)

            def global_decode():
                ctx.codec_decode(d_iout, icont, d_ioff, 4, (nblk, 8, 64), dct_quant.INDEX_CHUNK, d_idx)
                ctx.dctq_inverse(d_idx, shape, q, d_rec)
            row["global_step"] = {"q": q, "bits_per_voxel": rd["bits_per_voxel"], "cratio": 16.0 / rd["bits_per_voxel"],
                                  "lmax": rd["lmax"], "device_ms_int32_decode_plus_inverse": timed(ctx, global_decode)}
        else:
            row["global_step"] = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    for b in (d_den, d_rec, d_err, d_out, d_off, d_sz, d_idx, d_iout, d_ioff):
        b.free()
    return {"volume": list(shape), "seed": seed, "denoise_sigma": sigma, "chunk": list(chunk),
            "lossless": {"bits_per_voxel": 8.0 * lossless / n, "cratio": 2.0 * n / lossless,
                         "coded_bytes": int(lossless)},
            "global_step_note": "largest ladder step whose error is <= max_error in every chunk, one step for the "
                                "whole volume, indices coded as bench.py codes them (EXAC v2, 512 blocks x 8 x 64)",
            "rows": rows}


FG_DELTAS = (4, 8, 16)      # the bounds that get --fg-error rows


def _ms(times):
    return {"median": float(np.median(times)), "min": min(times), "max": max(times)}


def sweep_block(edge, deltas, sigma, fg_errors, seed=1000):
    """The store with a step per block next to the store with a step per chunk, on one denoised volume."""
    shape, chunk = (edge,) * 3, bench.CHUNK
    n = edge ** 3
    ctx = _native.context(0)
    d_noisy, d_den, d_rec = ctx.to_device(bench.synth_u16(shape, seed)), ctx.alloc(2 * n), ctx.alloc(2 * n)
    ctx.denoise_u16(d_noisy, d_den, shape, sigma, bench.OFFSET)
    ctx.sync()
    d_noisy.free()
    grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
    nchunks = int(np.prod(grid))
    nb, nbp = int(np.prod([c // 8 for c in chunk])), plane_bytes(chunk)
    den = d_den.download(shape, np.uint16)
    threshold = bench.OFFSET + 3.0 * sigma
    mask = (den > threshold).astype(np.uint8)
    fg_share = float(mask.mean())
    del den
    d_mask = ctx.to_device(mask.reshape(-1))
    del mask
    lossless, _ = ctx.codec_encode(d_den, 2, shape, chunk)
    d_err = ctx.alloc(4 * STEPS * nchunks)
    ladder = timed_all(ctx, lambda: ctx.dctq_ladder_errors(d_den, shape, chunk, d_err))
    cap = max(_native.bounded_volume_bound(shape, chunk), _native.block_bounded_volume_bound(shape, chunk))
    d_out, d_off, d_sz = ctx.alloc(cap), ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    d_plane = ctx.alloc(nbp * nchunks)
    rows = []
    for delta in deltas:
        v1_enc = timed_all(ctx, lambda: ctx.bounded_encode(d_den, shape, chunk, delta, out=d_out, out_capacity=cap,
                                                           offsets=d_off, sizes=d_sz, totals=False))
        v1_coded, v1_container = ctx.bounded_encode(d_den, shape, chunk, delta, out=d_out, out_capacity=cap,
                                                    offsets=d_off, sizes=d_sz)
        v1_dec = timed_all(ctx, lambda: ctx.bounded_decode(d_out, v1_container, d_off, shape, chunk, d_rec))
        per_chunk = {"bits_per_voxel": 8.0 * v1_coded / n, "coded_bytes": int(v1_coded),
                     "device_ms_ladder_kernel": _ms(ladder), "device_ms_encode": _ms(v1_enc),
                     "device_ms_decode": _ms(v1_dec)}
        for fg in [None] + [f for f in fg_errors if f <= delta and delta in FG_DELTAS]:
            m = None if fg is None else d_mask
            f = delta if fg is None else fg
            sel = timed_all(ctx, lambda: ctx.block_bounded_steps(d_den, shape, chunk, delta, f, d_plane, mask=m))
            enc = timed_all(ctx, lambda: ctx.block_bounded_encode(d_den, shape, chunk, delta, f, mask=m, out=d_out,
                                                                  out_capacity=cap, offsets=d_off, sizes=d_sz,
                                                                  totals=False))
            coded, container = ctx.block_bounded_encode(d_den, shape, chunk, delta, f, mask=m, out=d_out,
                                                        out_capacity=cap, offsets=d_off, sizes=d_sz)
            dec = timed_all(ctx, lambda: ctx.block_bounded_decode(d_out, container, d_off, shape, chunk, d_rec))
            err = ctx.masked_error_stats(d_rec, np.uint16, d_den, np.uint16, None, n)
            data = d_out.download((container,), np.uint8)
            offs = d_off.download((nchunks + 1,), np.uint64)
            mode1 = np.array([data[int(o) + 3] for o in offs[:-1]], dtype=bool)
            planes = np.stack([data[int(o) + 32:int(o) + 32 + nb] for o in offs[:-1][mode1]]) if mode1.any() \
                else np.zeros((0, nb), np.uint8)
            hist = np.bincount(planes.reshape(-1), minlength=256)
            p = hist[hist > 0] / max(1, planes.size)
            row = {"max_error": delta, "fg_max_error": fg, "bits_per_voxel": 8.0 * coded / n,
                   "cratio": 2.0 * n / coded, "coded_bytes": int(coded),
                   "bytes_vs_per_chunk": coded / v1_coded, "bytes_vs_lossless": coded / lossless,
                   "lmax": float(err[6]), "mae": float(err[1] / n),
                   "mode0_chunk_share": float(1.0 - mode1.mean()),
                   "verbatim_block_share_of_mode1_blocks": float(hist[0xFE] / max(1, planes.size)),
                   "step_histogram": {f"{float(LADDER[j]):g}": int(hist[j]) for j in range(STEPS) if hist[j]},
                   "step_plane_bits_per_voxel": 8.0 * nbp * int(mode1.sum()) / n,
                   "step_plane_order0_bits_per_voxel": float(-(p * np.log2(p)).sum()) * planes.size / n,
                   "device_ms_select_kernel": _ms(sel), "device_ms_encode": _ms(enc), "device_ms_decode": _ms(dec),
                   "select_vs_ladder_kernel": float(np.median(sel) / np.median(ladder)),
                   "encode_vs_per_chunk": float(np.median(enc) / np.median(v1_enc)),
                   "decode_vs_per_chunk": float(np.median(dec) / np.median(v1_dec)),
                   "per_chunk": per_chunk}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    for b in (d_den, d_rec, d_err, d_out, d_off, d_sz, d_plane, d_mask):
        b.free()
    return {"volume": list(shape), "seed": seed, "denoise_sigma": sigma, "chunk": list(chunk),
            "granularity": "block",
            "mask": f"denoised > offset + 3 sigma = {threshold:g} (the sweep's own choice)",
            "foreground_share": fg_share,
            "lossless": {"bits_per_voxel": 8.0 * lossless / n, "cratio": 2.0 * n / lossless,
                         "coded_bytes": int(lossless)},
            "timing_note": "HIP events; median, min and max of three repeats after one warm-up call; the per-chunk "
                           "figures are BoundedDctCodec's entries measured in the same session",
            "rows": rows}


PG_NOISE = {"gain": 4.0, "read_noise": 6.0, "offset": 37.0}     # its timing volume, its first quality row
PG_BRICK, PG_SLAB = 128, 8
PG_GENERATOR = ("clean: tests/util.py synth_volume((128, 128, 128), seed=3, pedestal=offset)[1], mirror-tiled to the "
                "volume; counts: tests/pg_pyref.py pg_volume(clean, gain, read_noise, offset, rng) per slab of 8 "
                "planes with rng = default_rng([7, slab]) -- the generator of the DESIGN.md 5.10 quality table, its "
                "clean brick tiled because synth_volume does not reach 1024^3")


def pg_bench_volume(shape, noise=PG_NOISE):
    """The uint16 Poisson-Gaussian volume ``PG_GENERATOR`` describes; slabs on host threads."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from pg_pyref import pg_volume
    from util import synth_volume
    brick = synth_volume((PG_BRICK,) * 3, seed=3, pedestal=noise["offset"])[1]

    def tile_axis(n):
        i = np.arange(n) % (2 * PG_BRICK)
        return np.where(i < PG_BRICK, i, 2 * PG_BRICK - 1 - i)

    iz, iy, ix = (tile_axis(n) for n in shape)
    out = np.empty(shape, dtype=np.uint16)

    def fill(k):
        z0, z1 = k * PG_SLAB, min((k + 1) * PG_SLAB, shape[0])
        clean = brick[iz[z0:z1]][:, iy][:, :, ix]
        out[z0:z1] = pg_volume(clean, noise["gain"], noise["read_noise"], noise["offset"], np.random.default_rng([7, k]))

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(fill, range(-(-shape[0] // PG_SLAB))))
    return out


def sweep_noise(edge, ks, volume_npy=None):
    """The store under a bound table from measured noise parameters next to the two constant bounds of its ends."""
    from aind_exaspim_image_compression.machine_learning.transforms import estimate_offset_device
    from aind_exaspim_image_compression.utils.noise import bound_table, estimate_poisson_gaussian
    shape, chunk = (edge,) * 3, bench.CHUNK
    n = edge ** 3
    if volume_npy and os.path.exists(volume_npy):
        vol = np.load(volume_npy)
        if vol.shape != shape or vol.dtype != np.uint16:
            raise SystemExit(f"{volume_npy} holds another volume")
    else:
        vol = pg_bench_volume(shape)
        if volume_npy:
            np.save(volume_npy, vol)
    ctx = _native.context(0)
    d_vol, d_rec = ctx.to_device(vol.reshape(-1)), ctx.alloc(2 * n)
    hist = ctx.u16_histogram(d_vol, n)
    p999 = int(np.searchsorted(np.cumsum(hist), 0.999 * n))
    offset = estimate_offset_device(ctx, d_vol, n)
    params = estimate_poisson_gaussian(d_vol, offset=offset, shape=shape, dtype=np.uint16)
    grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
    nchunks = int(np.prod(grid))
    nb, nbp = int(np.prod([c // 8 for c in chunk])), plane_bytes(chunk)
    lossless, _ = ctx.codec_encode(d_vol, 2, shape, chunk)
    cap = _native.block_bounded_volume_bound(shape, chunk)
    d_out, d_off, d_sz = ctx.alloc(cap), ctx.alloc(8 * (nchunks + 1)), ctx.alloc(4 * nchunks)
    d_plane = ctx.alloc(nbp * nchunks)

    def measure(delta, table, verify=False):
        """One store: ``delta`` everywhere (table None) or the table under max_error = 65535."""
        d_tab = None if table is None else ctx.to_device(table)
        sel = timed_all(ctx, lambda: ctx.block_bounded_steps(d_vol, shape, chunk, delta, delta, d_plane, table=d_tab),
                        reps=5)
        coded, container = ctx.block_bounded_encode(d_vol, shape, chunk, delta, delta, out=d_out, out_capacity=cap,
                                                    offsets=d_off, sizes=d_sz, table=d_tab)
        ctx.block_bounded_decode(d_out, container, d_off, shape, chunk, d_rec)
        err = ctx.masked_error_stats(d_rec, np.uint16, d_vol, np.uint16, None, n)
        data = d_out.download((container,), np.uint8)
        offs = d_off.download((nchunks + 1,), np.uint64)
        if d_tab is not None:
            d_tab.free()
        mode1 = np.array([data[int(o) + 3] for o in offs[:-1]], dtype=bool)
        planes = np.stack([data[int(o) + 32:int(o) + 32 + nb] for o in offs[:-1][mode1]]) if mode1.any() \
            else np.zeros((0, nb), np.uint8)
        h = np.bincount(planes.reshape(-1), minlength=256)
        row = {"max_error": int(delta), "bits_per_voxel": 8.0 * coded / n, "cratio": 2.0 * n / coded,
               "coded_bytes": int(coded), "bytes_vs_lossless": coded / lossless, "lmax": float(err[6]),
               "mae": float(err[1] / n), "mode0_chunk_share": float(1.0 - mode1.mean()),
               "verbatim_block_share_of_mode1_blocks": float(h[0xFE] / max(1, planes.size)),
               "step_histogram": {f"{float(LADDER[j]):g}": int(h[j]) for j in range(STEPS) if h[j]},
               "device_ms_select_kernel": _ms(sel)}
        if verify:                              # the guarantee itself, voxel by voxel, on the host
            rec = d_rec.download(shape, np.uint16)
            worst = -65535
            for z0 in range(0, edge, 64):
                v = vol[z0:z0 + 64]
                excess = np.abs(rec[z0:z0 + 64].astype(np.int32) - v) - table[v].astype(np.int32)
                worst = max(worst, int(excess.max()))
            row["largest_error_minus_bound"] = worst
        return row

    rows = []
    # the estimate is what a user has; the generator's own parameters show the bound under the true model
    for source, noise in (("estimated", params), ("generator", PG_NOISE)):
        pedestal = int(round(noise["offset"]))
        for k in ks:
            table = bound_table(noise, k)
            d_ped, d_999 = int(table[pedestal]), int(table[p999])
            row = {"noise": source, "k": k, "pedestal": pedestal, "table_at_pedestal": d_ped, "table_at_p999": d_999,
                   "table": measure(65535, table, verify=True),
                   "constant_at_pedestal": measure(d_ped, None),
                   "constant_at_p999": measure(d_999, None),
                   # the block decisions of the two rows above, through the table instantiation
                   "constant_table_at_pedestal": measure(65535, np.full(65536, d_ped, np.uint16)),
                   "constant_table_at_p999": measure(65535, np.full(65536, d_999, np.uint16))}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    for b in (d_vol, d_rec, d_out, d_off, d_sz, d_plane):
        b.free()
    return {"volume": list(shape), "chunk": list(chunk), "granularity": "block", "generator": PG_GENERATOR,
            "generator_noise": PG_NOISE, "estimated_noise": params,
            "pedestal_note": "the offset of the parameters in use, rounded: the estimate's offset is "
                             "transforms.estimate_offset, the 1st percentile of the non-zero counts",
            "p999_intensity": p999,
            "lossless": {"bits_per_voxel": 8.0 * lossless / n, "cratio": 2.0 * n / lossless,
                         "coded_bytes": int(lossless)},
            "timing_note": "HIP events around exabm4d_block_bounded_steps(_tab)_dev (plane memset + select kernel); "
                           "median, min and max of five repeats after one warm-up call, all in one session; "
                           "'table' and 'constant_table_at_*' run the table instantiation, 'constant_at_*' the "
                           "instantiation without a table",
            "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("edge", nargs="?", type=int, default=1024)
    ap.add_argument("deltas", nargs="?", default="1,2,4,8,16")
    ap.add_argument("sigma", nargs="?", type=float, default=bench.SIGMA)
    ap.add_argument("--granularity", choices=("chunk", "block"), default="chunk")
    ap.add_argument("--fg-error", default="", help="comma list of foreground bounds (block granularity only)")
    ap.add_argument("--noise-k", default="", help="comma list of k: bound = k noise standard deviations of the voxel "
                                                  "(block granularity only; deltas and sigma are not used)")
    ap.add_argument("--volume-npy", default="", help="with --noise-k: load the volume from this file if it exists, "
                                                     "else make it and save it there")
    a = ap.parse_args()
    deltas = [int(s) for s in a.deltas.split(",")]
    fg = [int(s) for s in a.fg_error.split(",") if s != ""]
    ks = [float(s) for s in a.noise_k.split(",") if s != ""]
    if ks:
        if a.granularity != "block" or fg:
            ap.error("--noise-k needs --granularity block and takes no --fg-error")
        print(json.dumps(sweep_noise(a.edge, ks, a.volume_npy or None), indent=1))
    elif a.granularity == "chunk":
        if fg:
            ap.error("--fg-error needs --granularity block")
        print(json.dumps(sweep(a.edge, deltas, a.sigma), indent=1))
    else:
        print(json.dumps(sweep_block(a.edge, deltas, a.sigma, fg), indent=1))


if __name__ == "__main__":
    main()
