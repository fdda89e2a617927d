"""BM4D on MI355X behind the call signature the reference uses.

The reference imports the third-party wheel (``from bm4d import bm4d``) and calls it as the
opaque two-argument function ``bm4d(raw, sigma)`` (reference machine_learning/data_handling.py:12,
:332, :926; evaluate.py:11, :202).  ``bm4d`` below accepts exactly that call; the work is done by
the HIP kernels of ``libexabm4d.so`` with the profile of BASELINE.json (8^3 blocks, step 4, 11^3
search window, groups of <= 16, 3-D DCT + Haar, hard-threshold stage then Wiener stage --
DESIGN.md section 3).  There is no CPU fallback.

Harness-level helpers mirror the reference's two call patterns (SURVEY.md section 8 row a-J):
``denoise_patches`` = scripts/precompute.py teacher generation (batch of fp32 patches -> clipped
teachers) and ``denoise_volume`` = uint16 volume in, uint16 volume out.

Placement (round 4).  The reference's pattern is a pool of forked workers, one ``bm4d(raw, sigma)`` per 64^3
patch (scripts/precompute.py:215-228).  Three ways to run it on an 8-GPU node, slowest first:
  * unchanged: every worker opens a context on ``_native.default_device()`` = its pool index mod the device
    count (``EXABM4D_DEVICE`` overrides) -- the pool spreads over the GPUs instead of piling onto device 0;
  * ``EXABM4D_BROKER=1`` (or ``broker.enable()`` in the parent): the workers never touch a GPU; one owner
    process per device coalesces their single patches into batched calls (``broker.py``);
  * ``denoise_patches(raw, sigma, devices="all")``: the whole batch split over all GPUs in one call.
All three give the same teachers, bit for bit (every patch carries its own fixed-point unit).
"""
import time
from dataclasses import dataclass, asdict

import numpy as np

from aind_exaspim_image_compression import _native


@dataclass(frozen=True)
class BM4DProfile:
    """Algorithm parameters (``exabm4d_params``).  Only the defaults' block / step / search /
    max_group values are implemented by the kernels; other values raise ``ValueError``."""

    block: int = 8
    step: int = 4
    search: int = 11
    max_group: int = 16
    lambda_ht: float = 2.7
    c_match_ht: float = 3.0
    c_match_wie: float = 0.6
    kaiser_beta: float = 2.0

    def native(self):
        return _native.default_params(**asdict(self))


_MAX_VOXELS_PER_CALL = 1 << 30     # ~21 GB of device scratch for the two-stage pipeline


def _denoise_batched(device, arr, sigma, params, stages, clip):
    """One device call per sub-batch of volumes (the reference's cache build runs 30 000
    patches, scripts/precompute.py:278-319; they do not have to fit the GPU at once).  With the broker
    enabled (and no explicit device) the calls go to the device's owner process instead of a context of
    this process."""
    from aind_exaspim_image_compression import broker
    if device is None and broker.enabled():
        def run(a):
            return broker.denoise(a, sigma, params, stages, clip)
    else:
        ctx = _native.context(device)

        def run(a):
            return ctx.denoise_f32_host(a, sigma, params=params, stages=stages, clip=clip)
    if arr.ndim == 3 or arr.shape[0] * arr[0].size <= _MAX_VOXELS_PER_CALL:
        return run(arr)
    per = max(1, _MAX_VOXELS_PER_CALL // arr[0].size)
    out = np.empty(arr.shape, dtype=np.float32)
    for i in range(0, arr.shape[0], per):
        out[i:i + per] = run(arr[i:i + per])
    return out


def _stages(stage_arg):
    if stage_arg in (None, "all", "ALL_STAGES", 2):
        return 2
    if stage_arg in ("ht", "hard_thresholding", "HARD_THRESHOLDING", 1):
        return 1
    raise ValueError(f"unknown stage_arg: {stage_arg!r}")


def _sigma(sigma, vol, device=None, **resident):
    """``sigma`` as a float.  The string "auto" is measured from ``vol`` on the device (``utils/noise.py``:
    Donoho's pooled estimator on the Haar HHH detail of 2x2x2 cells) -- here, at the top of the
    call, so that only floats travel to the broker and to worker processes."""
    if not isinstance(sigma, str):
        return float(np.asarray(sigma).reshape(-1)[0])
    from aind_exaspim_image_compression.utils import noise
    return noise.resolve_sigma(sigma, vol, device=device, **resident)


def _pg_noise(noise, inverse, sigma, offset, vol=None, resident=None):
    """The ``exabm4d_pg_noise`` of a ``noise=`` argument, or None when ``noise`` is None.

    ``noise``: ``{"gain", "read_noise", "offset"}`` (what ``utils.noise.estimate_poisson_gaussian`` returns), an
    anscombe transform cfg, or "auto": measured once on the whole volume -- the noise curve on ``resident`` (the
    uploaded volume, where there is one), the offset by ``transforms.estimate_offset`` on the host array ``vol``.
    The model carries the noise level and the pedestal, so ``sigma`` must be None and ``offset`` left alone."""
    if noise is None:
        if sigma is None:
            raise ValueError("give sigma (a number or 'auto'), or noise= for Poisson-Gaussian data")
        return None
    if sigma is not None:
        raise ValueError("give either sigma or noise=, not both: under noise= the stabilised data has sigma 1")
    if offset not in (None, 0, 0.0):
        raise ValueError("with noise= the offset is the model's: leave offset= alone")
    from aind_exaspim_image_compression.utils import noise as noise_mod
    if isinstance(noise, str):
        if noise != "auto":
            raise ValueError("noise must be a dict, an anscombe cfg or 'auto', not %r" % noise)
        if vol is None:
            raise ValueError("noise='auto' needs the counts as a host array")
        from aind_exaspim_image_compression.machine_learning.transforms import estimate_offset
        off = estimate_offset(vol)
        if resident is None:
            noise = noise_mod.estimate_poisson_gaussian(vol, offset=off)
        else:
            noise = noise_mod.estimate_poisson_gaussian(resident, offset=off, shape=vol.shape, dtype=np.uint16)
    return _native.pg_noise(inverse=inverse, **noise_mod.pg_params(noise))


def bm4d(z, sigma_psd, profile=None, stage_arg=None, device=None):
    """Denoise a 3-D volume (or a 4-D batch of volumes) with two-stage BM4D.

    ``z``: array of counts, any real dtype (computed in float32, like the reference's patches:
    data_handling.py:353); ``sigma_psd``: noise standard deviation in the same units, or "auto" for
    ``utils.noise.estimate_sigma(z)`` (one value for the whole batch).  Returns a
    new float32 array of the same shape, NOT clipped (the reference clips at its call site,
    data_handling.py:333)."""
    arr = np.asarray(z)
    if arr.ndim not in (3, 4):
        raise ValueError("bm4d expects a 3-D volume or a 4-D batch of volumes")
    sigma = _sigma(sigma_psd, arr, device)
    prof = profile or BM4DProfile()
    return _denoise_batched(device, arr.astype(np.float32, copy=False), sigma, prof.native(),
                            _stages(stage_arg), None)


def split_batch(n, parts):
    """[start, stop) of ``parts`` near-equal consecutive shares of ``n`` items (empty shares dropped)."""
    parts = max(1, min(int(parts), int(n))) if n > 0 else 1
    edges = [(n * i) // parts for i in range(parts + 1)]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _device_share(args):
    """Child process of ``denoise_patches(..., devices=...)``: one device, one share of the batch, data in
    the parent's shared-memory segments."""
    from multiprocessing import shared_memory
    name_in, name_out, shape, a, b, sigma, max_count, prof, device = args
    seg_in, seg_out = shared_memory.SharedMemory(name=name_in), shared_memory.SharedMemory(name=name_out)
    try:
        src = np.ndarray(shape, dtype=np.float32, buffer=seg_in.buf)
        dst = np.ndarray(shape, dtype=np.float32, buffer=seg_out.buf)
        dst[a:b] = _denoise_batched(device, src[a:b], float(sigma), BM4DProfile(**prof).native(), 2,
                                    (0.0, float(max_count)))
        del src, dst
    finally:
        seg_in.close()
        seg_out.close()
    return b - a


def _denoise_patches_pg(raw, nz, prof, device):
    """uint16 patches [N, Z, Y, X] through the batch form of the stabilised pipeline, sub-batches of at most
    _MAX_VOXELS_PER_CALL voxels."""
    raw = np.ascontiguousarray(raw, dtype=np.uint16)
    if raw.ndim == 3:
        raw = raw[None]
    if raw.ndim != 4:
        raise ValueError("denoise_patches(noise=...) expects uint16 patches [N, Z, Y, X]")
    ctx = _native.context(device)
    per = max(1, _MAX_VOXELS_PER_CALL // raw[0].size)
    out = np.empty(raw.shape, dtype=np.uint16)
    for i in range(0, raw.shape[0], per):
        part = raw[i:i + per]
        d_in = ctx.to_device(part)
        d_out = ctx.alloc(part.nbytes)
        try:
            ctx.denoise_pg_u16(d_in, d_out, part.shape[1:], nz, params=prof.native(), stages=2, batch=part.shape[0])
            ctx.sync()
            out[i:i + per] = d_out.download(part.shape, np.uint16)
        finally:
            d_in.free()
            d_out.free()
    return out


def denoise_patches(raw, sigma=None, max_count=65535.0, profile=None, device=None, devices=None, noise=None,
                    inverse="closed_form"):
    """``teacher = np.clip(bm4d(raw, sigma), 0, max_count)`` for a batch ``raw[N, Z, Y, X]`` of
    offset-subtracted float32 patches, in one device call (reference call pattern:
    data_handling.py:331-333 inside scripts/precompute.py:215-228).

    ``devices``: "all" or a list of device indices -- the batch is cut into one consecutive share per
    entry and every share runs in a FRESH child process that owns that device (started with the ``spawn``
    method: nothing is forked after HIP has been initialised, and this process never touches a GPU for the
    call); the patches travel through shared memory and come back in order.  Patches are independent units
    (no halo, no collective) and each carries its own fixed-point unit, so the result equals the
    single-device call bit for bit.  ``sigma="auto"`` is measured in THIS process (on ``device``, or the default
    one) before the batch is cut: the shares only ever see the float.

    ``noise=``: ``raw`` holds uint16 COUNTS (pedestal included) under Poisson-Gaussian noise;
    the patches go through the stabilised pipeline's batch form in this process and come back as uint16 counts.
    ``sigma`` must then be None; "auto" measures the model over the whole batch as one population.  ``devices=``
    and the broker do not carry a noise model: combined with ``noise=`` they raise."""
    if noise is not None:
        from aind_exaspim_image_compression import broker
        if devices is not None or (device is None and broker.enabled()):
            raise ValueError("denoise_patches: noise= runs in this process; it cannot be combined with devices= "
                             "or the broker")
        counts = np.ascontiguousarray(raw, dtype=np.uint16)
        return _denoise_patches_pg(counts, _pg_noise(noise, inverse, sigma, None, vol=counts),
                                   profile or BM4DProfile(), device)
    _pg_noise(None, inverse, sigma, None)
    raw = np.asarray(raw, dtype=np.float32)
    if raw.ndim == 3:
        raw = raw[None]
    prof = profile or BM4DProfile()
    sigma = _sigma(sigma, raw, device)      # "auto": measured once, over the whole batch, before any split
    if devices is None:
        return _denoise_batched(device, raw, float(sigma), prof.native(), 2, (0.0, float(max_count)))
    if device is not None:
        raise ValueError("denoise_patches: give either device or devices")
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError("devices must be 'all' or a list of device indices")
        devices = list(range(max(1, _native.device_count_no_init())))
    devices = [int(d) for d in devices]
    if not devices:
        raise ValueError("devices is empty")
    import multiprocessing
    from multiprocessing import shared_memory
    shares = split_batch(raw.shape[0], len(devices))
    seg_in = shared_memory.SharedMemory(create=True, size=max(1, raw.nbytes))
    seg_out = shared_memory.SharedMemory(create=True, size=max(1, raw.nbytes))
    try:
        np.ndarray(raw.shape, dtype=np.float32, buffer=seg_in.buf)[...] = raw
        jobs = [(seg_in.name, seg_out.name, raw.shape, a, b, float(sigma), float(max_count), asdict(prof), d)
                for (a, b), d in zip(shares, devices)]
        mp = multiprocessing.get_context("spawn")
        with mp.Pool(len(jobs)) as pool:
            done = pool.map(_device_share, jobs, chunksize=1)
        if sum(done) != raw.shape[0]:
            raise RuntimeError("denoise_patches: a device share did not complete")
        return np.ndarray(raw.shape, dtype=np.float32, buffer=seg_out.buf).copy()
    finally:
        for seg in (seg_in, seg_out):
            seg.close()
            seg.unlink()


def denoise_volume(vol_u16, sigma=None, offset=0.0, profile=None, stages=2, device=None, noise=None,
                   inverse="closed_form"):
    """uint16 volume -> uint16 volume: ``(float)v - offset`` -> BM4D -> ``+ offset`` -> clip to
    [0, 65535] -> rint -> uint16, entirely on the device (read_counts + bm4d + clip + the
    rint/uint16 cast of IntensityTransform.inverse).  The uint16 form matches its second stage on the basic
    estimate rounded to counts: both matching passes are 16-bit integer work.  ``sigma="auto"``
    measures it on the uploaded volume (``utils.noise.estimate_sigma``).

    ``noise=`` instead of ``sigma`` is for sCMOS data, whose noise grows with the signal
    (``var = gain (mean - offset) + read_noise^2``): the counts are variance-stabilised, denoised at sigma 1 in
    the fp32 kernels and inverted, in one device call.  ``noise`` is a dict ``{"gain", "read_noise", "offset"}``
    (``utils.noise.estimate_poisson_gaussian``), an anscombe transform cfg, or "auto" (measured here, once);
    ``inverse``: "closed_form" (exact unbiased, the default), "asymptotic" or "algebraic"."""
    vol = np.ascontiguousarray(vol_u16, dtype=np.uint16)
    if vol.ndim != 3:
        raise ValueError("denoise_volume expects a 3-D uint16 volume")
    prof = profile or BM4DProfile()
    ctx = _native.context(device)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    try:
        nz = _pg_noise(noise, inverse, sigma, offset, vol=vol, resident=d_in)
        if nz is not None:
            ctx.denoise_pg_u16(d_in, d_out, vol.shape, nz, params=prof.native(), stages=int(stages))
            ctx.sync()
            return d_out.download(vol.shape, np.uint16)
        sigma = _sigma(sigma, d_in, shape=vol.shape, dtype=np.uint16)
        ctx.denoise_u16(d_in, d_out, vol.shape, float(sigma), float(offset), params=prof.native(),
                        stages=int(stages))
        ctx.sync()
        return d_out.download(vol.shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()


def denoise_chunked(vol_u16, sigma=None, offset=0.0, chunk=256, halo=8, profile=None, stages=2,
                    device=None, noise=None, inverse="closed_form"):
    """Chunk-local mode of BASELINE.json config 4: the volume is tiled by ``chunk``^3 cores, every
    core is read with ``halo`` voxels on each side -- the read window is CUT where the volume ends,
    nothing is padded or replicated at the faces (SURVEY.md appendix A item 11's
    "edge clamping" is read as clamping the window, and the oracle processes the identical
    truncated arrays) -- and denoised in isolation -- independent units, like the reference's one-``bm4d``-call-per-patch
    pool (scripts/precompute.py:215-228) -- and only the cores are written.  One batched device
    call (``exabm4d_denoise_chunked_u16_dev``); uint16 in, uint16 out.  ``sigma="auto"`` measures it once on the
    uploaded volume, not per chunk.  ``noise=`` / ``inverse=`` as in ``denoise_volume``: every padded chunk goes
    through the stabilised pipeline (``exabm4d_denoise_pg_chunked_u16_dev``); "auto" is measured once on the
    whole volume."""
    vol = np.ascontiguousarray(vol_u16, dtype=np.uint16)
    if vol.ndim != 3:
        raise ValueError("denoise_chunked expects a 3-D uint16 volume")
    prof = profile or BM4DProfile()
    ctx = _native.context(device)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    try:
        nz = _pg_noise(noise, inverse, sigma, offset, vol=vol, resident=d_in)
        if nz is not None:
            ctx.denoise_pg_chunked_u16(d_in, d_out, vol.shape, nz, chunk=int(chunk), halo=int(halo),
                                       params=prof.native(), stages=int(stages))
            ctx.sync()
            return d_out.download(vol.shape, np.uint16)
        sigma = _sigma(sigma, d_in, shape=vol.shape, dtype=np.uint16)
        ctx.denoise_chunked_u16(d_in, d_out, vol.shape, float(sigma), float(offset),
                                chunk=int(chunk), halo=int(halo), params=prof.native(),
                                stages=int(stages))
        ctx.sync()
        return d_out.download(vol.shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()


def denoise_chunked_streamed(vol_u16, sigma=None, offset=0.0, chunk=256, halo=8, profile=None, stages=2,
                             device=None, out=None, noise=None, inverse="closed_form"):
    """``denoise_chunked`` for volumes that should not (or cannot) sit on the device whole -- the
    reference's production harness denoises whole images (scripts/evaluate_bm4dnet.py:51-181), and
    BASELINE config 4's tile is 64 GiB.  ``vol_u16`` is a C-contiguous uint16 array or ``np.memmap``;
    layers of chunks travel up, are denoised chunk by chunk in isolation and travel down while the
    next layer is in the kernels (``exabm4d_denoise_chunked_u16_host``).  ``out`` may name the
    destination (another array / writeable memmap of the same shape); the result equals
    ``denoise_chunked`` on the whole volume.  ``noise=`` / ``inverse=`` as in ``denoise_volume``; "auto" uploads
    the whole volume once to measure it, so for a volume that does not fit the device measure a sample with
    ``utils.noise.estimate_poisson_gaussian`` and pass the dict."""
    vol = vol_u16 if isinstance(vol_u16, np.ndarray) and vol_u16.dtype == np.uint16 and \
        vol_u16.flags.c_contiguous else np.ascontiguousarray(vol_u16, dtype=np.uint16)
    if vol.ndim != 3:
        raise ValueError("denoise_chunked_streamed expects a 3-D uint16 volume")
    if out is None:
        out = np.empty(vol.shape, dtype=np.uint16)
    _native.check_host_volume_pair(vol, out)
    prof = profile or BM4DProfile()
    nz = _pg_noise(noise, inverse, sigma, offset, vol=vol)
    ctx = _native.context(device)
    if nz is not None:
        ctx.denoise_pg_chunked_u16_host(vol, out, nz, chunk=int(chunk), halo=int(halo), params=prof.native(),
                                        stages=int(stages))
        return out
    ctx.denoise_chunked_u16_host(vol, out, float(sigma), float(offset), chunk=int(chunk), halo=int(halo),
                                 params=prof.native(), stages=int(stages))
    return out


def _core_runs(n, chunk, halo):
    """Per core along an axis of ``n`` voxels: (start, extent, halo in front, halo behind), the halo cut at the
    faces -- ``chunk_runs`` of ``csrc/api_bm4d.hip``."""
    runs = []
    for start in range(0, n, chunk):
        e = min(chunk, n - start)
        runs.append((start, e, min(halo, start), min(halo, n - (start + e))))
    return runs


# device bytes a core costs while its brick is in flight, per voxel of its padded window (the pipeline's scratch --
# keys, numerator, basic estimate, corner weights, two fp32 volumes and the Wiener pair: 40 bytes -- plus the fp32 and
# uint16 copies and the window batch in and out) and per voxel of the core (its pool and coded streams)
_STORE_WINDOW_BYTES = 56
_STORE_CORE_BYTES = 8


def denoise_store(src, dst_path, sigma=None, offset=0.0, chunk=256, halo=8, profile=None, stages=2, device=None,
                  noise=None, inverse="closed_form", codec=None, chunks=None, attributes=None, budget_bytes=4 << 30,
                  stats=None):
    """A stored volume in, a denoised and coded store out, without ever holding the volume: the result is
    ``write_zarr(denoise_chunked(read_zarr(src)[0, 0], ...), dst_path, ...)``, chunk file for chunk file, for a
    volume of any size.

    ``src``: a store's path or a ``StoredArray``.  The destination is made with ``chunk_store.create_zarr``
    (``codec``: default ``ExacCodec(2)``; ``chunks``: default the source's; ``attributes``).  The cores of the
    chunk-local mode (``chunk``^3 voxels, read with ``halo`` voxels on each side, the window cut at
    the volume's faces) are visited in raster order, in bricks of as many cores as fit ``budget_bytes`` of device
    memory (at least one).  A brick's windows are read from the source per window shape
    (``read_patches(out="device")``), every shape is denoised by one batched pipeline call -- the pipeline
    ``denoise_chunked`` runs, on the same padded arrays -- and the cores are scattered into one pool of destination
    chunks, coded and committed.  ``chunk`` must be a multiple of the destination's chunk shape on every axis, so that
    every destination chunk lies in one core and none is read back.

    ``sigma`` / ``offset`` / ``noise`` / ``inverse`` as in ``denoise_chunked``, except that "auto" is rejected: nothing
    here sees the whole volume.  Measure the store first, in one pass out of core -- ``m =
    utils.noise.measure_store(src)`` -- and pass ``sigma=m.sigma()`` or ``noise=m.poisson_gaussian()``.

    Returns raw bytes / stored chunk bytes, like ``write_zarr``.  ``stats`` (a dict) receives ``seconds`` per phase
    (read, denoise, scatter, encode, files_write), ``bricks``, ``windows`` and ``largest_alloc``, the largest device
    allocation made here (the pipeline's scratch is the context's and is not counted)."""
    from aind_exaspim_image_compression.utils import chunk_store, store_windows
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    # -- every argument check, before a context exists
    if isinstance(sigma, str) or isinstance(noise, str):
        raise ValueError("denoise_store: 'auto' is not available, nothing here sees the whole volume; measure the "
                         "store first (m = utils.noise.measure_store(src)) and pass m.sigma() or m.poisson_gaussian()")
    nz_model = _pg_noise(noise, inverse, sigma, offset)
    chunk, halo, stages = int(chunk), int(halo), int(stages)
    if chunk < 1 or not 0 <= halo <= 64:
        raise ValueError("denoise_store: chunk >= 1 and 0 <= halo <= 64")
    if stages not in (1, 2):
        raise ValueError("denoise_store: stages must be 1 or 2")
    if int(budget_bytes) < 1:
        raise ValueError("denoise_store: budget_bytes must be positive")
    chunks = store_windows.check_chunks(chunks)
    arr = src if hasattr(src, "read_patches") else chunk_store.open_zarr(src, device=device)
    shape = arr.shape[2:]
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    if any(chunk % c for c in chunks[2:]):
        raise ValueError("denoise_store: chunk=%d is not a multiple of the destination's chunk shape %s on every "
                         "axis" % (chunk, chunks[2:]))
    runs = [_core_runs(n, chunk, halo) for n in shape]
    if any(e + lo + hi < 8 for axis in runs for _, e, lo, hi in axis):
        raise ValueError("denoise_store: a padded chunk would be thinner than one block (8)")
    codec = codec or ExacCodec(2)
    prof = (profile or BM4DProfile()).native()
    sigma = None if nz_model is not None else float(np.asarray(sigma).reshape(-1)[0])

    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=device)
    # cores in raster order: (window start, window shape, core offset in the window, core start, core extent)
    cores = []
    for z0, ez, lz, hz in runs[0]:
        for y0, ey, ly, hy in runs[1]:
            for x0, ex, lx, hx in runs[2]:
                cores.append(((z0 - lz, y0 - ly, x0 - lx), (ez + lz + hz, ey + ly + hy, ex + lx + hx), (lz, ly, lx),
                              (z0, y0, x0), (ez, ey, ex)))
    cost = [_STORE_WINDOW_BYTES * int(np.prod(c[1])) + _STORE_CORE_BYTES * int(np.prod(c[4])) for c in cores]
    budget = int(budget_bytes)
    reader = budget // store_windows.READER_SHARE
    bricks, first, held = [], 0, 0
    for n, c in enumerate(cost):
        if n > first and held + c > budget - reader:
            bricks.append((first, n))
            first, held = n, 0
        held += c
    bricks.append((first, len(cores)))

    largest, windows = 0, 0
    with store_windows.capped_pools([arr], budget):
        ctx = _native.context(device)
        clock = store_windows.PhaseClock(("read", "denoise", "scatter", "encode", "files_write"), True, ctx.sync)
        seconds = clock.seconds
        with store_windows.BrickSink("denoise_store", out, ctx, shape, chunks, box="core") as sink:
            for b0, b1 in bricks:
                brick = cores[b0:b1]
                classes = {}
                for k, c in enumerate(brick):
                    classes.setdefault(c[1], []).append(k)
                with sink.pool([c[3] for c in brick], [c[4] for c in brick]) as pool:
                    largest = max(largest, 2 * pool.g.pool_elems)
                    for win, members in classes.items():
                        nvox = int(np.prod(win))
                        t0 = time.perf_counter()
                        d_in = arr.read_patches([brick[k][0] for k in members], win, is_center=False, out="device")
                        try:
                            with ctx.alloc(2 * nvox * len(members)) as d_res:
                                largest = max(largest, 2 * nvox * len(members))
                                t1 = time.perf_counter()
                                if nz_model is not None:
                                    ctx.denoise_pg_u16(d_in, d_res, win, nz_model, params=prof, stages=stages,
                                                       batch=len(members))
                                else:
                                    ctx.denoise_u16(d_in, d_res, win, sigma, float(offset), params=prof, stages=stages,
                                                    batch=len(members))
                                t2 = clock()
                                # the cores: the inner part of each window, its front offset its own
                                rec = np.zeros(len(members), dtype=_native.BOX_SRC)
                                remap = np.full(len(brick) + 1, -1, dtype=np.int32)      # [-1] stays -1
                                for j, k in enumerate(members):
                                    _, _, (lz, ly, lx), org, ext = brick[k]
                                    rec[j]["base"] = j * nvox + (lz * win[1] + ly) * win[2] + lx
                                    rec[j]["stride_z"], rec[j]["stride_y"] = win[1] * win[2], win[2]
                                    rec[j]["z0"], rec[j]["y0"], rec[j]["x0"] = org
                                    rec[j]["ez"], rec[j]["ey"], rec[j]["ex"] = ext
                                    remap[k] = j
                                pool.scatter(d_res, nvox * len(members), np.uint16, rec,
                                             dst_boxes=remap[pool.g.dst_boxes])
                                t3 = clock()
                        finally:
                            d_in.free()
                        seconds["read"] += t1 - t0
                        seconds["denoise"] += t2 - t1
                        seconds["scatter"] += t3 - t2
                        windows += len(members)
                    pool.commit()
    if stats is not None:
        stats.update(sink.finish(seconds), seconds=seconds, bricks=len(bricks), windows=windows, largest_alloc=largest)
    return 2 * int(np.prod(shape)) / sink.written
