"""Denoising under Poisson-Gaussian noise on the GPU: the two streams, the whole stabilised
pipeline, its chunk-local and streamed forms and the Python surface, every result bit for bit against
tests/pg_pyref.py composed with the oracle's fp32 pipeline:

    quantise(pg_pyref.inverse(oracle.bm4d(pg_pyref.forward(v), 1.0, stages)))

Shapes are the smallest that reach every path: one block (8^3), clamped grid positions with an odd row length
(9 x 13 x 18: the one-wave matching kernel, the narrow normalisation), a volume with several tiles per axis and
nx % 4 == 0 (24 x 20 x 28: the wide normalisation with the fused inverse), and a batch of two."""
import ctypes
import functools

import numpy as np
import pytest

import pg_pyref as P
from util import GuardedView, synth_volume

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.bm4d import (denoise_chunked, denoise_chunked_streamed, denoise_patches,
                                                 denoise_volume)
from aind_exaspim_image_compression.utils import noise as N

pytestmark = pytest.mark.gpu
F32 = np.float32
PARAMS = [(4.0, 6.0, 37.0), (20.0, 3.0, 37.0), (1.5, 8.0, 100.0), (1.0, 0.0, 0.0)]
KINDS = ["closed_form", "asymptotic", "algebraic"]


def as_dict(p):
    return {"gain": p[0], "read_noise": p[1], "offset": p[2]}


def pg_counts(shape, params, seed):
    """Poisson-Gaussian counts on synth_volume's clean signal, with voxels forced to 0, to values below the
    offset and to 65535 (C order positions, so every shape has them)."""
    gain, rn, off = params
    _, clean = synth_volume(shape, seed=seed, pedestal=off)
    v = P.pg_volume(clean, gain, rn, off, np.random.default_rng(100 + seed)).reshape(-1)
    v[3::97] = 0
    v[5::89] = np.uint16(max(int(off) - 9, 0))
    v[11::211] = np.uint16(max(int(off) - 1, 0))
    v[7::301] = 65535
    return v.reshape(shape)


# ---- parity hooks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
def test_forward_stream(ctx, params):
    nz = _native.pg_noise(*params)
    allv = np.arange(65536, dtype=np.uint16)
    want = P.forward(allv, params)
    np.testing.assert_array_equal(N.stabilise(allv, as_dict(params)), want)
    rng = np.random.default_rng(1)
    for n in (1, 7, 8, 9, 4099):                      # the 8-per-lane body, its tail, and misaligned views
        data = rng.integers(0, 65536, n).astype(np.uint16)
        for k_in, k_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
            src = GuardedView(ctx, np.uint16, n, k_in, data)
            dst = GuardedView(ctx, np.float32, n, k_out)
            try:
                ctx.gat_forward_u16(nz, src.ptr, dst.ptr, n)
                ctx.sync()
                dst.check_output(want[data], f"forward n={n} views {k_in},{k_out}")
                src.check_untouched(f"forward n={n}")
            finally:
                src.free()
                dst.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params", PARAMS)
def test_inverse_stream(ctx, params, kind):
    c = P.Consts(*params)
    top = float(P.forward(np.array([65535], np.uint16), c)[0])
    edges = np.array([0.0, c.d0, np.nextafter(c.d0, F32(np.inf)), np.nextafter(c.d0, F32(-np.inf))], dtype=F32)
    D = np.concatenate([np.linspace(-1.0, top + 1.0, 100001).astype(F32), edges])
    want = P.inverse(D, c, kind)
    np.testing.assert_array_equal(N.unstabilise(D, as_dict(params), kind), want)
    nz = _native.pg_noise(*params, inverse=kind)
    src = GuardedView(ctx, np.float32, D.size, 1, D)         # a misaligned view: one voxel per lane
    dst = GuardedView(ctx, np.uint16, D.size, 1)
    try:
        ctx.gat_inverse_u16(nz, src.ptr, dst.ptr, D.size)
        ctx.sync()
        dst.check_output(want, "inverse, views +1")
        src.check_untouched("inverse")
    finally:
        src.free()
        dst.free()


# ---- whole pipeline -----------------------------------------------------------------------------------------------
# (shape, batch, parameter set): every parameter set denoises something
CASES = {"one_block": ((8, 8, 8), 1, PARAMS[1]), "clamped_odd": ((9, 13, 18), 1, PARAMS[2]),
         "tiles": ((24, 20, 28), 1, PARAMS[0]), "batch2": ((16, 16, 16), 2, PARAMS[3])}


@functools.lru_cache(maxsize=None)
def case_volumes(name):
    """The case's counts [batch, z, y, x]."""
    shape, batch, params = CASES[name]
    vols = np.stack([pg_counts(shape, params, seed=10 * list(CASES).index(name) + b) for b in range(batch)])
    vols.setflags(write=False)
    return vols


_ESTIMATES = {}


def stabilised_estimate(oracle, name, stages, b):
    """The oracle's fp32 pipeline at sigma 1 on the stabilised volume b of a case: computed once, shared by the
    three inverses and the Python-surface tests, read-only."""
    key = (name, stages, b)
    if key not in _ESTIMATES:
        e = oracle.bm4d(P.forward(case_volumes(name)[b], CASES[name][2]), 1.0, stages=stages)
        e.setflags(write=False)
        _ESTIMATES[key] = e
    return _ESTIMATES[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_whole_pipeline(ctx, oracle, name, stages, kind):
    shape, batch, params = CASES[name]
    vols = case_volumes(name)
    want = np.stack([P.inverse(stabilised_estimate(oracle, name, stages, b), params, kind) for b in range(batch)])
    d_in = ctx.to_device(vols)
    d_out = ctx.alloc(vols.nbytes).fill(0xA5)
    try:
        ctx.denoise_pg_u16(d_in, d_out, shape, _native.pg_noise(*params, inverse=kind), stages=stages, batch=batch)
        ctx.sync()
        got = d_out.download(vols.shape, np.uint16)
    finally:
        d_in.free()
        d_out.free()
    np.testing.assert_array_equal(got, want)
    assert np.any(got != vols)                       # it denoised something


def test_profile_accounts_for_the_forward_stream(ctx):
    shape, _, params = CASES["tiles"]
    vol = pg_counts(shape, params, seed=1)
    ctx.set_option("profile", 1)
    try:
        d_in = ctx.to_device(vol)
        d_out = ctx.alloc(vol.nbytes)
        ctx.denoise_pg_u16(d_in, d_out, shape, _native.pg_noise(*params))
        ms = ctx.profile_read()
        d_in.free()
        d_out.free()
    finally:
        ctx.set_option("profile", 0)
    for phase in ("counts_from_u16", "blockmatch_ht", "stage_ht", "blockmatch_wie", "stage_wie", "normalize_out"):
        assert ms[phase] > 0.0, (phase, ms)


# ---- chunk-local and streamed -------------------------------------------------------------------------------------
def test_chunked_and_streamed(ctx, oracle):
    """40 x 36 x 44 in 16^3 cores with an 8-voxel halo: 27 padded chunks of twelve shapes, the windows cut at the
    faces; the expectation is the composition on every truncated padded chunk (oracle.padded_chunks), as
    tests/test_chunked_gpu.py builds its own."""
    params = PARAMS[0]
    vol = pg_counts((40, 36, 44), params, seed=4)
    want = P.denoise_chunked(oracle, vol, params, 16, 8)
    got = denoise_chunked(vol, noise=as_dict(params), chunk=16, halo=8)
    np.testing.assert_array_equal(got, want)
    streamed = denoise_chunked_streamed(vol, noise=as_dict(params), chunk=16, halo=8)
    np.testing.assert_array_equal(streamed, got)
    # a chunk that covers the volume with halo 0 is the whole-volume call
    np.testing.assert_array_equal(denoise_chunked(vol, noise=as_dict(params), chunk=64, halo=0),
                                  denoise_volume(vol, noise=as_dict(params)))


@pytest.mark.parametrize("kind,stages", [("closed_form", 2), ("asymptotic", 1)])
def test_chunked_ragged_odd(ctx, oracle, kind, stages):
    """20 x 33 x 17 in 16^3 cores: ragged one-voxel cores along y and x, an odd row length.

    With halo = 4 the last chunks along y and x are 1 + 4 = 5 voxels thick, thinner than one 8^3 block, which no
    BM4D pipeline here (or the oracle) processes: the call is refused like the uint16 chunked form refuses it.
    With halo = 8 they are 9 thick and the result is compared."""
    params = PARAMS[2]
    vol = pg_counts((20, 33, 17), params, seed=6)
    with pytest.raises(ValueError, match="thinner than one block"):
        denoise_chunked(vol, noise=as_dict(params), chunk=16, halo=4, inverse=kind, stages=stages)
    with pytest.raises(ValueError, match="thinner than one block"):
        denoise_chunked(vol, 24.0, params[2], chunk=16, halo=4, stages=stages)
    want = P.denoise_chunked(oracle, vol, params, 16, 8, kind, stages)
    np.testing.assert_array_equal(denoise_chunked(vol, noise=as_dict(params), chunk=16, halo=8, inverse=kind,
                                                  stages=stages), want)
    np.testing.assert_array_equal(denoise_chunked_streamed(vol, noise=as_dict(params), chunk=16, halo=8,
                                                           inverse=kind, stages=stages), want)


# ---- Python surface -----------------------------------------------------------------------------------------------
def test_python_surface(ctx, oracle):
    shape, _, params = CASES["tiles"]
    vol = case_volumes("tiles")[0]
    want = P.inverse(stabilised_estimate(oracle, "tiles", 2, 0), params, "closed_form")
    np.testing.assert_array_equal(denoise_volume(vol, noise=as_dict(params)), want)
    cfg = {"kind": "anscombe", "params": as_dict(params)}
    np.testing.assert_array_equal(denoise_volume(vol, noise=cfg, inverse="asymptotic"),
                                  P.inverse(stabilised_estimate(oracle, "tiles", 2, 0), params, "asymptotic"))
    for bad in (dict(sigma=24.0, noise=as_dict(params)), dict(noise=as_dict(params), offset=37.0), dict(),
                dict(noise="guess"), dict(noise=as_dict(params), inverse="exact"),
                dict(noise={"gain": 1.0, "read_noise": 2.0}), dict(noise={"kind": "asinh", "params": {}})):
        with pytest.raises(ValueError):
            denoise_volume(vol, **bad)
    with pytest.raises(ValueError):
        denoise_chunked(vol, 24.0, noise=as_dict(params))
    with pytest.raises(ValueError):
        denoise_chunked_streamed(vol, 24.0, noise=as_dict(params))
    # the old path, untouched
    v24, _ = synth_volume(shape, seed=3, as_u16=True)
    np.testing.assert_array_equal(denoise_volume(v24, 24.0, offset=37.0), oracle.bm4d_u16(v24, 24.0, 37.0))


def test_noise_auto(ctx):
    """noise="auto" measures the model once on the uploaded volume: the call with estimate_poisson_gaussian(v)."""
    gain, rn, off = PARAMS[0]
    levels = off + np.array([0.0, 40.0, 160.0, 640.0, 2560.0, 10240.0])
    clean = np.repeat(levels, 8)[:, None, None] * np.ones((1, 32, 32))
    vol = P.pg_volume(clean, gain, rn, off, np.random.default_rng(11))
    model = N.estimate_poisson_gaussian(vol)
    assert model["gain"] > 0.0 and set(model) == {"gain", "read_noise", "offset"}
    print("auto model:", model)
    np.testing.assert_array_equal(denoise_volume(vol, noise="auto"), denoise_volume(vol, noise=model))
    np.testing.assert_array_equal(denoise_chunked(vol, noise="auto", chunk=32, halo=8),
                                  denoise_chunked(vol, noise=model, chunk=32, halo=8))


def test_denoise_patches(ctx, oracle):
    shape, batch, params = CASES["batch2"]
    vols = case_volumes("batch2")
    want = np.stack([P.inverse(stabilised_estimate(oracle, "batch2", 2, b), params) for b in range(batch)])
    got = denoise_patches(vols, noise=as_dict(params))
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        denoise_patches(vols, noise=as_dict(params), devices=[0])
    with pytest.raises(ValueError):
        denoise_patches(vols, 1.0, noise=as_dict(params))


# ---- bad input ----------------------------------------------------------------------------------------------------
def test_bad_structs_are_refused_before_a_launch(ctx):
    lib = _native.lib()
    p = _native.default_params()
    vol = pg_counts((8, 8, 8), PARAMS[0], seed=2)
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes).fill(0xA5)
    d_f32 = ctx.alloc(vol.size * 4).fill(0xA5)
    bad = []
    for field, value in (("gain", 0.0), ("gain", -1.0), ("gain", float("nan")), ("gain", float("inf")),
                         ("read_noise", -0.5), ("read_noise", float("nan")), ("offset", float("nan")),
                         ("offset", 1e6), ("size", 16), ("size", 24), ("inverse", 3), ("inverse", -1)):
        s = _native.pg_noise(*PARAMS[0])
        setattr(s, field, value)
        bad.append((field, value, s))
    try:
        for field, value, s in bad:
            what = f"{field} = {value}"
            assert lib.exabm4d_denoise_pg_u16_dev(ctx.handle, d_in.ptr, d_out.ptr, 8, 8, 8, 1, ctypes.byref(s),
                                                  ctypes.byref(p), 2) == -1, what
            assert lib.exabm4d_last_error(ctx.handle), what
            assert lib.exabm4d_denoise_pg_chunked_u16_dev(ctx.handle, d_in.ptr, d_out.ptr, 8, 8, 8, 0, 8, 8, 0,
                                                          ctypes.byref(s), ctypes.byref(p), 2) == -1, what
            host_out = np.full(vol.shape, 0xA5A5, np.uint16)
            assert lib.exabm4d_denoise_pg_chunked_u16_host(ctx.handle, vol.ctypes.data, host_out.ctypes.data, 8, 8, 8,
                                                           8, 0, ctypes.byref(s), ctypes.byref(p), 2) == -1, what
            assert np.all(host_out == 0xA5A5), what
            assert lib.exabm4d_gat_forward_u16_dev(ctx.handle, ctypes.byref(s), d_in.ptr, d_f32.ptr, vol.size) == -1, what
            assert lib.exabm4d_gat_inverse_u16_dev(ctx.handle, ctypes.byref(s), d_f32.ptr, d_out.ptr, vol.size) == -1, what
        assert lib.exabm4d_denoise_pg_u16_dev(ctx.handle, d_in.ptr, d_out.ptr, 8, 8, 8, 1, None, ctypes.byref(p), 2) == -1
        ctx.sync()
        assert np.all(d_out.download(vol.shape, np.uint16) == 0xA5A5)          # nothing was launched
        assert np.all(d_f32.download((vol.size,), np.uint32) == 0xA5A5A5A5)
        # and the context is fine afterwards
        ctx.denoise_pg_u16(d_in, d_out, (8, 8, 8), _native.pg_noise(*PARAMS[0]))
        ctx.sync()
        assert np.any(d_out.download(vol.shape, np.uint16) != 0xA5A5)
    finally:
        for b in (d_in, d_out, d_f32):
            b.free()
