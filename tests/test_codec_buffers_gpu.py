"""The codec entries of the C-ABI (csrc/api_codec.hip: chunk byte histograms, DCT quantiser, EXAC v1 / v2 chunk coder,
error-bounded codec) on poisoned, guarded and offset device buffers.

Every device argument is a ``GuardedView`` (tests/util.py): the data at an element offset inside a larger buffer whose
other bytes hold a fill pattern, 0xA5 in one run and 0x00 in the other.  Outputs must equal the expected bytes under
both fills -- a decoder that skipped a voxel would leave the fill there, and no earlier allocation's content can stand
in for a result -- every byte around an output must come back as uploaded, and every input must come back unchanged.
Expected values: oracle.codec_oracle.encode per chunk, the original array for decodes, the oracle's dctq_forward /
dctq_inverse, tests/bounded_pyref.py, numpy for the histograms.  All comparisons are equalities.

Alignment each argument needs, from the loads and stores the kernels make through it (include/exabm4d.h states the
same, and the offsets used here follow it):

* ``vol`` of every entry (uint16 / int32 input): element-wise loads everywhere -- chunk_hist_kernel,
  dctq_forward_kernel, load_pair (bq_ladder / bq_forward), rans2_model_kernel, rans2_model_strips_kernel,
  rans2_model_rows32_kernel, rans2_code_kernel, rans_encode_kernel's pass 2 -- except rans_encode_kernel's (EXAC v1) histogram pass, which loads
  a uint4 per lane from addresses that are 4-byte aligned, and only where the kernel itself found
  ``(vol + base * TS) % 4 == 0`` on a chunk of whole 64-element rows; elsewhere it takes the one-element-per-lane pass.
  Global 16-byte loads need no more than that on gfx950, and the suite's v1 volumes with nx = 130 have always taken
  them from such addresses.  Natural alignment (2 / 4 bytes) suffices.
* decoded ``vol``: byte stores (rans_decode_kernel), in-place uint32 load / store for int32 (unzigzag_kernel),
  element stores (rans2_decode_kernel, dctq_inverse_kernel, bq_inverse_kernel).  Natural alignment.
* ``idx``, ``err``, ``hist``, ``sizes_dev``: 4-byte element loads / stores / atomics.  ``offsets_dev``: 8-byte.
* ``out``: uint16 stores from a multiple of 16 (rans_pack_kernel, rans2_pack_kernel) would do with 2 bytes, but
  bq_copy_kernel stores uint4; both encoders refuse an ``out`` that is not 16-byte aligned (check_container).
* ``in``: uint32 header loads at multiples of 16 (+ 32 behind a bounded header) and uint16 word loads in the EXAC
  decoders, uint4 header loads in bq_parse_kernel; both decoders refuse an ``in`` that is not 16-byte aligned.

No entry needed a new check: the two arguments that need more than their natural alignment are already refused."""
import numpy as np
import pytest

import bounded_pyref as ref
from test_bounded_codec_gpu import flat_and_textured
from test_codec_gpu import denoised_like
from util import GuardedView, synth_volume

from aind_exaspim_image_compression import _native
from oracle import codec_oracle as co

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x00)
VERSIONS = pytest.mark.parametrize("version", [2, 1])
# element offsets from a 16-byte boundary: (input vol, decoded vol, sizes_dev, offsets_dev, idx / err / hist)
LAYOUTS_U16 = [(0, 0, 0, 0, 0), (1, 3, 1, 1, 3), (3, 1, 3, 0, 1), (2, 2, 0, 1, 0)]
LAYOUTS_I32 = LAYOUTS_U16[:3]
OUT_K = 16                      # containers sit 16 bytes past the guard: 16-byte aligned, not the buffer's start

U16_CASES = [
    ((1, 1, 1), (1, 1, 1)),
    ((5, 6, 7), (4, 4, 4)),            # ragged on every axis, rows narrower than a wave
    ((9, 40, 12), (9, 40, 12)),        # v2 taps several x-rows up
    ((3, 5, 1000), (2, 5, 300)),       # rows straddle chunk rows
    ((6, 10, 320), (4, 6, 128)),       # whole 64-element rows: v1's wide histogram pass at even k, narrow at odd k
    ((3, 5, 1001), (3, 5, 1001)),      # odd nx
    ((2, 3, 9000), (2, 3, 9000)),      # beyond v2's tap limit
    ((65, 66, 128), (64, 64, 64)),     # v2's strips kernel (cx = 64, nx % 64 = 0), ragged z and y
    ((8, 16, 64), (8, 16, 64)),        # incompressible: the longest streams the bound has to hold
]
I32_CASES = [
    ((3, 8, 64), (512, 8, 64)),
    ((515, 8, 64), (512, 8, 64)),      # one full and one 3-block chunk through rans2_model_rows32_kernel
    ((1, 1, 5000), (1, 1, 4096)),
]
EXTREMES = np.array([0, -1, 1, -2 ** 30, 2 ** 30, 255, -256, 65536, -2 ** 31, 2 ** 31 - 1], dtype=np.int32)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        if isinstance(_cache[key], np.ndarray):
            _cache[key].setflags(write=False)
    return _cache[key]


def u16_volume(shape):
    def make():
        if shape == (8, 16, 64):
            return np.random.default_rng(2).integers(0, 65536, shape).astype(np.uint16)
        vol = denoised_like(shape, seed=sum(shape))
        vol.reshape(-1)[:: max(1, vol.size // 11)] = 65535
        return vol
    return cached(("u16", shape), make)


def i32_volume(oracle, shape):
    """Quantisation indices of a synthetic volume (the oracle's), with the extreme values of
    test_quantisation_indices_int32 spread over them."""
    def make():
        n = int(np.prod(shape))
        src = synth_volume((8, 8, 8 * -(-n // 512)), seed=n, as_u16=True)[0]
        flat = oracle.dctq_forward(src, 2.0).reshape(-1)[:n].copy()
        step = n // len(EXTREMES) - 1
        flat[5:5 + step * len(EXTREMES):step] = EXTREMES
        return flat.reshape(shape)
    return cached(("i32", shape), make)


def layout_container(streams):
    """-> (container bytes [0, offsets[-1]) with zero pads, offsets u64 [n + 1], sizes u32 [n])."""
    sizes = np.array([len(s) for s in streams], dtype=np.uint32)
    offsets = np.zeros(len(streams) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15))
    data = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for s, o in zip(streams, offsets[:-1]):
        data[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return data, offsets, sizes


def exac_expected(vol, chunk, version):
    return cached(("exac", vol.dtype.str, vol.shape, chunk, version),
                  lambda: layout_container([co.encode(c, version=version) for c in co.chunks(vol, chunk)]))


class Views:
    """GuardedViews of one case, freed together."""

    def __init__(self, ctx, fill):
        self.ctx, self.fill, self.all = ctx, fill, []

    def __call__(self, dtype, n, k, data=None):
        v = GuardedView(self.ctx, dtype, n, k, data, fill=self.fill)
        self.all.append(v)
        return v

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for v in self.all:
            v.free()


def check_container(v_out, v_off, v_sz, totals, want, what):
    """Streams and zeroed pads over [0, offsets[-1]) of the view (what lies behind, up to out_capacity, is
    unspecified), offsets, sizes, totals, and not a byte around any of the three views."""
    data, offsets, sizes = want
    assert totals == (int(sizes.sum()), int(offsets[-1])), what
    v_sz.check_output(sizes, f"{what}: sizes_dev")
    v_off.check_output(offsets, f"{what}: offsets_dev")
    v_out.check_output(data, f"{what}: container", upto=data.size)


def run_exac(ctx, vol, chunk, version, fill, ks):
    """Encode into a container of exactly the bound, sizes-only mode, decode of that container: one layout, one fill."""
    k_vol, k_dec, k_sz, k_off, _ = ks
    ts, shape = vol.dtype.itemsize, vol.shape
    want = exac_expected(vol, chunk, version)
    data, offsets, sizes = want
    cap = _native.codec_volume_bound(ts, shape, chunk)
    assert data.size <= cap
    what = f"EXAC v{version} {vol.dtype} {shape}/{chunk} fill {fill:#x} offsets {ks}"
    with Views(ctx, fill) as view:
        v_in = view(vol.dtype, vol.size, k_vol, vol)
        v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, sizes.size + 1, k_off)
        v_sz = view(np.uint32, sizes.size, k_sz)
        totals = ctx.codec_encode(v_in.ptr, ts, shape, chunk, out=v_out.ptr, out_capacity=cap, offsets=v_off.ptr,
                                  sizes=v_sz.ptr, version=version)
        check_container(v_out, v_off, v_sz, totals, want, what)
        v_sz2 = view(np.uint32, sizes.size, k_sz)
        assert ctx.codec_encode(v_in.ptr, ts, shape, chunk, sizes=v_sz2.ptr, version=version) == totals
        v_sz2.check_output(sizes, f"{what}: sizes only")
        v_in.check_untouched(f"{what}: vol")
        # in_bytes is the container length exactly: the fill, not zeros, lies behind it
        v_cont, v_offin = view(np.uint8, data.size, OUT_K, data), view(np.uint64, offsets.size, k_off, offsets)
        v_dec = view(vol.dtype, vol.size, k_dec)
        ctx.codec_decode(v_cont.ptr, data.size, v_offin.ptr, ts, shape, chunk, v_dec.ptr)
        v_dec.check_output(vol, f"{what}: decoded vol")
        v_cont.check_untouched(f"{what}: in")
        v_offin.check_untouched(f"{what}: offsets_dev of the decoder")


@VERSIONS
@pytest.mark.parametrize("shape,chunk", U16_CASES)
def test_exac_uint16_on_guarded_offset_buffers(ctx, oracle, shape, chunk, version):
    """Streams, pads, offsets, sizes and totals equal the oracle's at every offset and fill, with out_capacity the
    bound exactly; the decode of the container into a poisoned view is the input, voxel for voxel."""
    vol = u16_volume(shape)
    for fill in FILLS:
        for ks in LAYOUTS_U16:
            run_exac(ctx, vol, chunk, version, fill, ks)


@VERSIONS
@pytest.mark.parametrize("shape,chunk", I32_CASES)
def test_exac_int32_on_guarded_offset_buffers(ctx, oracle, shape, chunk, version):
    vol = i32_volume(oracle, shape)
    for fill in FILLS:
        for ks in LAYOUTS_I32:
            run_exac(ctx, vol, chunk, version, fill, ks)


def test_v1_histogram_narrow_pass_at_odd_element_offsets(ctx, oracle):
    """EXAC v1 on a uint16 volume of whole 64-element rows ((6, 10, 320) in (4, 6, 128) chunks, so ex = 128 or 64 and
    nx is even).  rans_encode_kernel picks its histogram pass by ``wide = fast && (TS == 4 || nx % 2 == 0) &&
    ((uintptr_t)vol + b.base * TS) % 4 == 0``.  With the volume at an even element offset (k = 0, 2) that holds and
    pass 1 loads 16 bytes per lane; at an odd one (k = 1, 3) the address is 2 mod 4, ``wide`` is false although the
    rows are whole, and the one-element-per-lane pass of the ``else`` branch runs with ``fast`` row cursors -- the
    branch no hipMalloc'ed volume of this shape reaches.  Both must count the same histograms: streams, sizes and
    the decode are those of the oracle at every k."""
    shape, chunk = (6, 10, 320), (4, 6, 128)
    vol = u16_volume(shape)
    for fill in FILLS:
        for k in (1, 3, 0, 2):
            run_exac(ctx, vol, chunk, 1, fill, (k, k, 0, 0, 0))


# ---- DCT quantiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1.0, 37.5])
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 8), (7, 8, 9), (8, 8, 24), (20, 17, 33)])
def test_dct_quantiser_on_guarded_offset_buffers(ctx, oracle, shape, q):
    """(8, 8, 8): nbx = 1, the pair's second block is the clamped first; (8, 8, 24) and (20, 17, 33): odd nbx.  The
    inverse's guard starts right behind the last voxel: a store for a voxel of the blocks' overhang shows there."""
    vol = cached(("dct", shape), lambda: synth_volume(shape, seed=sum(shape), as_u16=True)[0])
    idx = oracle.dctq_forward(vol, q)
    rec = oracle.dctq_inverse(idx, shape, q)
    for fill in FILLS:
        for k_vol, k_dec, _, _, k_idx in LAYOUTS_U16:
            what = f"{shape} q {q} fill {fill:#x} offsets {(k_vol, k_dec, k_idx)}"
            with Views(ctx, fill) as view:
                v_in, v_idx = view(np.uint16, vol.size, k_vol, vol), view(np.int32, idx.size, k_idx)
                ctx.dctq_forward(v_in.ptr, shape, q, v_idx.ptr)
                ctx.sync()
                v_idx.check_output(idx, f"dctq_forward {what}")
                v_in.check_untouched(f"dctq_forward {what}")
                v_idxin, v_dec = view(np.int32, idx.size, k_idx, idx), view(np.uint16, vol.size, k_dec)
                ctx.dctq_inverse(v_idxin.ptr, shape, q, v_dec.ptr)
                ctx.sync()
                v_dec.check_output(rec, f"dctq_inverse {what}")
                v_idxin.check_untouched(f"dctq_inverse {what}")


# ---- error-bounded codec ---------------------------------------------------------------------------------------------
def two_mode_volume():
    return np.ascontiguousarray(flat_and_textured()[:16, :16, :])


BOUNDED_CASES = [((1, 1, 1), (64, 64, 64)), ((7, 8, 9), (64, 64, 64)), ((8, 8, 8), (8, 8, 8)),
                 ((20, 17, 33), (8, 16, 24)),          # multi-chunk, ragged; both modes at a bound of 4
                 ((16, 16, 128), (16, 16, 64))]        # a flat and a textured chunk of test_bounded_codec_gpu's volume


def bounded_volume(shape):
    def make():
        if shape == (16, 16, 128):
            return two_mode_volume()
        # little noise, so that a bound of 4 leaves (20, 17, 33) chunks of either mode; saturating and zero voxels
        vol = synth_volume(shape, seed=sum(shape), sigma=1.0, as_u16=True)[0]
        flat = vol.reshape(-1)
        flat[:: max(1, flat.size // 9)] = 65535
        flat[3:: max(1, flat.size // 7)] = 0
        return vol
    return cached(("bq", shape), make)


def bounded_ladder(vol, chunk):
    return cached(("bq-ladder", vol.shape, chunk), lambda: ref.volume_ladder(vol, chunk))


def bounded_expected(vol, chunk, delta):
    def make():
        streams, rec, steps = ref.encode_volume(vol, chunk, delta, bounded_ladder(vol, chunk))
        return layout_container(streams), rec, steps
    return cached(("bq-enc", vol.shape, chunk, delta), make)


@pytest.mark.parametrize("shape,chunk", BOUNDED_CASES)
def test_ladder_errors_on_guarded_offset_buffers(ctx, oracle, shape, chunk):
    vol = bounded_volume(shape)
    errs = bounded_ladder(vol, chunk)
    for fill in FILLS:
        for k_vol, _, _, _, k_err in LAYOUTS_U16:
            what = f"ladder {shape}/{chunk} fill {fill:#x} offsets {(k_vol, k_err)}"
            with Views(ctx, fill) as view:
                v_in, v_err = view(np.uint16, vol.size, k_vol, vol), view(np.uint32, errs.size, k_err)
                ctx.dctq_ladder_errors(v_in.ptr, shape, chunk, v_err.ptr)
                ctx.sync()
                v_err.check_output(errs, what)
                v_in.check_untouched(what)


@pytest.mark.parametrize("delta", [0, 4])
@pytest.mark.parametrize("shape,chunk", BOUNDED_CASES)
def test_bounded_codec_on_guarded_offset_buffers(ctx, oracle, shape, chunk, delta):
    """Streams and pads equal the restatement's with out_capacity the bound exactly; the decode into a poisoned view
    is the restatement's reconstruction and within the bound of the input."""
    vol = bounded_volume(shape)
    want, rec, steps = bounded_expected(vol, chunk, delta)
    data, offsets, sizes = want
    if shape == (16, 16, 128):       # bound 0: the flat chunk lossy, the textured one lossless; bound 4: two steps
        assert (steps[0] is not None and steps[1] is None) if delta == 0 else steps[0] > steps[1] >= 0, steps
    if shape == (20, 17, 33) and delta == 4:
        assert None in steps and len(set(steps)) > 2, steps
    assert int(np.abs(rec.astype(np.int64) - vol).max()) <= delta
    cap = _native.bounded_volume_bound(shape, chunk)
    assert data.size <= cap
    for fill in FILLS:
        for ks in LAYOUTS_U16:
            k_vol, k_dec, k_sz, k_off, _ = ks
            what = f"bounded {shape}/{chunk} max_error {delta} fill {fill:#x} offsets {ks}"
            with Views(ctx, fill) as view:
                v_in = view(np.uint16, vol.size, k_vol, vol)
                v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, offsets.size, k_off)
                v_sz = view(np.uint32, sizes.size, k_sz)
                totals = ctx.bounded_encode(v_in.ptr, shape, chunk, delta, out=v_out.ptr, out_capacity=cap,
                                            offsets=v_off.ptr, sizes=v_sz.ptr)
                check_container(v_out, v_off, v_sz, totals, want, what)
                v_sz2 = view(np.uint32, sizes.size, k_sz)
                assert ctx.bounded_encode(v_in.ptr, shape, chunk, delta, sizes=v_sz2.ptr) == totals
                v_sz2.check_output(sizes, f"{what}: sizes only")
                v_in.check_untouched(f"{what}: vol")
                v_cont, v_offin = view(np.uint8, data.size, OUT_K, data), view(np.uint64, offsets.size, k_off, offsets)
                v_dec = view(np.uint16, vol.size, k_dec)
                ctx.bounded_decode(v_cont.ptr, data.size, v_offin.ptr, shape, chunk, v_dec.ptr)
                v_dec.check_output(rec, f"{what}: decoded vol")
                v_cont.check_untouched(f"{what}: in")
                v_offin.check_untouched(f"{what}: offsets_dev of the decoder")


# ---- chunk byte histograms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,chunk", [((5, 6, 7), (4, 4, 4)), ((3, 5, 1000), (2, 5, 300))])
def test_chunk_byte_histograms_on_guarded_offset_buffers(ctx, shape, chunk):
    vol = u16_volume(shape)
    want = np.stack([np.concatenate([np.bincount(c.reshape(-1) & 255, minlength=256),
                                     np.bincount(c.reshape(-1) >> 8, minlength=256)])
                     for c in co.chunks(vol, chunk)]).astype(np.uint32)
    for fill in FILLS:
        for k_vol, k_hist in ((0, 0), (1, 3), (3, 1)):
            what = f"histograms {shape}/{chunk} fill {fill:#x} offsets {(k_vol, k_hist)}"
            with Views(ctx, fill) as view:
                v_in, v_hist = view(np.uint16, vol.size, k_vol, vol), view(np.uint32, want.size, k_hist)
                ctx.chunk_byte_histograms(v_in.ptr, shape, chunk, v_hist.ptr)
                ctx.sync()
                v_hist.check_output(want, what)
                v_in.check_untouched(what)


# ---- refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ["exac", "bounded"])
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx, oracle, codec):
    """A misaligned out, an out_capacity one below the bound, an out without offsets_dev and a misaligned in raise
    ValueError; the poisoned outputs are as uploaded afterwards, and the next good call gives the oracle's bytes."""
    shape, chunk = ((5, 6, 7), (4, 4, 4)) if codec == "exac" else ((20, 17, 33), (8, 16, 24))
    vol = u16_volume(shape) if codec == "exac" else bounded_volume(shape)
    if codec == "exac":
        want, rec = exac_expected(vol, chunk, 2), vol
        cap = _native.codec_volume_bound(2, shape, chunk)

        def encode(v_in, **kw):
            return ctx.codec_encode(v_in.ptr, 2, shape, chunk, version=2, **kw)

        def decode(data, nbytes, off, dec):
            ctx.codec_decode(data, nbytes, off, 2, shape, chunk, dec)
    else:
        want, rec, _ = bounded_expected(vol, chunk, 4)
        cap = _native.bounded_volume_bound(shape, chunk)

        def encode(v_in, **kw):
            return ctx.bounded_encode(v_in.ptr, shape, chunk, 4, **kw)

        def decode(data, nbytes, off, dec):
            ctx.bounded_decode(data, nbytes, off, shape, chunk, dec)
    data, offsets, sizes = want
    with Views(ctx, 0xA5) as view:
        v_in = view(np.uint16, vol.size, 1, vol)
        v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, offsets.size, 0)
        v_sz = view(np.uint32, sizes.size, 0)
        with pytest.raises(ValueError, match="out must be 16-byte aligned"):
            encode(v_in, out=v_out.ptr + 8, out_capacity=cap, offsets=v_off.ptr, sizes=v_sz.ptr)
        with pytest.raises(ValueError, match="out_capacity is below"):
            encode(v_in, out=v_out.ptr, out_capacity=cap - 1, offsets=v_off.ptr, sizes=v_sz.ptr)
        with pytest.raises(ValueError, match="offsets_dev is required"):
            encode(v_in, out=v_out.ptr, out_capacity=cap, sizes=v_sz.ptr)
        ctx.sync()
        for v in (v_in, v_out, v_off, v_sz):
            v.check_untouched(f"{codec}: refused encode")
        check_container(v_out, v_off, v_sz, encode(v_in, out=v_out.ptr, out_capacity=cap, offsets=v_off.ptr,
                                                   sizes=v_sz.ptr), want, f"{codec}: encode after the refusals")
        # the container 8 bytes into a 16-byte aligned region: inside the buffer, misaligned
        v_cont, v_offin = view(np.uint8, data.size + 8, OUT_K, np.concatenate([np.zeros(8, np.uint8), data])), \
            view(np.uint64, offsets.size, 0, offsets)
        v_dec = view(np.uint16, vol.size, 1)
        with pytest.raises(ValueError, match="in must be 16-byte aligned"):
            decode(v_cont.ptr + 8, data.size, v_offin.ptr, v_dec.ptr)
        ctx.sync()
        for v in (v_cont, v_offin, v_dec):
            v.check_untouched(f"{codec}: refused decode")
        v_good = view(np.uint8, data.size, OUT_K, data)
        decode(v_good.ptr, data.size, v_offin.ptr, v_dec.ptr)
        v_dec.check_output(rec, f"{codec}: decode after the refusal")
