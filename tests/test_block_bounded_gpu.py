"""Error-bounded codec with a step per 8^3 block and a per-voxel bound on the MI355X against
tests/block_bounded_pyref.py: streams byte for byte, the decode voxel for voxel, and the guarantee
|decoded - input| <= where(mask, fg_max_error, max_error) checked directly.  All comparisons are equalities."""
import numpy as np
import pytest

import block_bounded_pyref as ref
from test_codec_buffers_gpu import OUT_K, Views, check_container, layout_container
from util import synth_volume

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec

pytestmark = pytest.mark.gpu

RAGGED = ((20, 17, 40), (16, 16, 32))       # ragged on every axis, lbx odd in the x-edge chunks, outside blocks
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _frozen(a):
    a.setflags(write=False)
    return a


def volume(name):
    def make():
        if name == "ragged":
            return _frozen(synth_volume(RAGGED[0], seed=2, sigma=3.0, as_u16=True)[0])
        if name == "voxel":
            return _frozen(np.full((1, 1, 1), 4242, np.uint16))
        if name == "constant":
            return _frozen(np.full((9, 9, 9), 1000, np.uint16))
        if name == "checker":
            z, y, x = np.meshgrid(np.arange(8), np.arange(16), np.arange(24), indexing="ij")
            return _frozen((((z + y + x) & 1) * 65535).astype(np.uint16))
        assert name == "chunks64"
        return _frozen(synth_volume((64, 64, 128), seed=5, sigma=3.0, as_u16=True)[0])
    return cached(("vol", name), make)


def mask_of(name, kind):
    """None, or a uint8 mask derived from the restatement and the synthetic volume's clean signal, never from the code
    under test."""
    if kind is None:
        return None

    def make():
        vol = volume(name)
        if kind == "zero":
            return _frozen(np.zeros(vol.shape, np.uint8))
        if kind == "all":
            return _frozen(np.full(vol.shape, 3, np.uint8))            # any non-zero value is foreground
        if name == "chunks64":
            return _frozen((synth_volume((64, 64, 128), seed=5, sigma=3.0, as_u16=True)[1] > 67).astype(np.uint8))
        # the voxels of every block the restatement finds verbatim at a bound of 0, plus the voxel [12, 3, 20]
        assert name == "ragged" and kind == "verbatim"
        shape, chunk = RAGGED
        m = np.zeros(shape, np.uint8)
        for st, s in zip(ref.volume_steps(vol, chunk, 0), ref.chunk_slices(shape, chunk)):
            for bz, by, bx in zip(*np.nonzero(st == -1)):
                z0, y0, x0 = s[0].start + 8 * bz, s[1].start + 8 * by, s[2].start + 8 * bx
                m[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = 1
        assert m.any()
        m[12, 3, 20] = 1
        return _frozen(m)
    return cached(("mask", name, kind), make)


#        volume      chunk          max_error  fg_max_error  mask
CASES = [("ragged", RAGGED[1], d, None, None) for d in (0, 1, 4, 16)] + \
        [("ragged", RAGGED[1], d, f, "verbatim") for d, f in ((16, 0), (4, 0), (4, 1))] + \
        [("voxel", (8, 8, 8), 4, None, None),
         ("constant", (16, 16, 16), 4, None, None),
         ("checker", (8, 16, 24), 16, None, None),
         ("ragged", RAGGED[1], 4, 0, "zero"),
         ("ragged", RAGGED[1], 16, 4, "all"),
         ("chunks64", (64, 64, 64), 8, 0, "clean")]
IDS = [f"{n}-{d}-{f}-{m}" for n, _, d, f, m in CASES]


def expected(case):
    """-> ((container, offsets, sizes), streams, reconstruction, step planes) of the restatement, computed once."""
    name, chunk, delta, delta_fg, kind = case

    def make():
        streams, rec, planes = ref.encode_volume(volume(name), chunk, delta, delta_fg, mask_of(name, kind))
        return layout_container(streams), streams, _frozen(rec), planes
    return cached(("enc",) + case, make)


def bound_of(case):
    name, _, delta, delta_fg, kind = case
    m = mask_of(name, kind)
    return np.full(volume(name).shape, delta) if m is None else np.where(m != 0, delta_fg, delta)


def codec_of(case):
    return BlockBoundedCodec(case[2], case[3])


def test_the_cases_reach_every_kind_of_chunk_and_block(oracle):
    """From the restatement's output alone: the cases hold chunks of either mode, verbatim blocks inside mode-1
    chunks, outside blocks and many different steps -- what the comparisons below then cover."""
    modes0 = verbatim = outside = 0
    steps = set()
    for case in CASES:
        for p in expected(case)[3]:
            if p is None:
                modes0 += 1
                continue
            verbatim += int((p == -1).sum())
            outside += int((p == -2).sum())
            steps |= set(p[p >= 0].tolist())
    assert modes0 >= 1 and verbatim >= 1 and outside >= 1 and len(steps) >= 8, (modes0, verbatim, outside, steps)
    # what DESIGN.md 3.10c records of the ragged volume
    shape, chunk = RAGGED
    assert all(p is None for p in expected(("ragged", chunk, 0, None, None))[3])
    for d in (16, 4):
        planes = expected(("ragged", chunk, d, 0, "verbatim"))[3]
        assert int((planes[0] == -1).sum()) == 5 and planes[1] is None


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_streams_and_decode_equal_the_restatement(oracle, case):
    name, chunk, delta, delta_fg, kind = case
    vol, mask = volume(name), mask_of(name, kind)
    (data, offsets, sizes), streams, rec, planes = expected(case)
    codec = codec_of(case)
    enc = codec.encode_volume(vol, chunk, mask=mask)
    assert len(enc.sizes) == len(streams)
    for i, s in enumerate(streams):
        assert enc.chunk_bytes(i) == s, f"chunk {i}"
    np.testing.assert_array_equal(enc.offsets, offsets)
    assert np.all(enc.offsets % 16 == 0)
    np.testing.assert_array_equal(enc.data, data)                       # the padding between the streams too
    np.testing.assert_array_equal(codec.encode_volume(vol, chunk, mask=mask, want_bytes=False).sizes, sizes)
    np.testing.assert_array_equal(codec.chunk_sizes(vol, chunk, mask=mask), sizes)
    got = BlockBoundedCodec.block_steps(enc)
    for a, b in zip(got, planes):
        assert (a is None and b is None) or np.array_equal(a, b)
    dec = codec.decode_volume(enc)
    assert dec.dtype == np.uint16 and dec.shape == vol.shape
    np.testing.assert_array_equal(dec, rec)
    err = np.abs(dec.astype(np.int64) - vol.astype(np.int64))
    assert np.all(err <= bound_of(case)), f"largest excess {int((err - bound_of(case)).max())}"
    if delta == 0:
        np.testing.assert_array_equal(dec, vol)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "ragged" and c[4] in (None, "verbatim")],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] == "ragged" and c[4] in (None, "verbatim")])
def test_select_steps_of_every_chunk(oracle, case):
    """The step planes alone, mode-0 chunks included (at a bound of 0 every chunk of this volume is one)."""
    name, chunk, delta, delta_fg, kind = case
    vol, mask = volume(name), mask_of(name, kind)
    want = np.stack(ref.volume_steps(vol, chunk, delta, delta_fg, mask))
    got = codec_of(case).select_steps(vol, chunk, mask=mask)
    assert got.dtype == np.int16 and got.shape == ref.grid(vol.shape, chunk) + tuple(c // 8 for c in chunk)
    np.testing.assert_array_equal(got.reshape(want.shape), want)


def test_uniform_masks_equal_the_unmasked_streams(oracle):
    """An all-zero mask gives the streams of no mask, an all-foreground one those of BlockBoundedCodec(fg_max_error)."""
    vol, chunk = volume("ragged"), RAGGED[1]
    none4 = BlockBoundedCodec(4).encode_volume(vol, chunk)
    zero = BlockBoundedCodec(4, 0).encode_volume(vol, chunk, mask=mask_of("ragged", "zero"))
    np.testing.assert_array_equal(zero.data, none4.data)
    np.testing.assert_array_equal(zero.sizes, none4.sizes)
    full = BlockBoundedCodec(16, 4).encode_volume(vol, chunk, mask=mask_of("ragged", "all"))
    np.testing.assert_array_equal(full.data, none4.data)
    np.testing.assert_array_equal(full.sizes, none4.sizes)
    assert none4.data.tobytes() == expected(("ragged", chunk, 4, None, None))[0][0].tobytes()


def test_one_chunk_encode_and_decode(oracle):
    """``encode`` / ``decode`` of single chunks: the nominal chunk shape is the extent rounded up to multiples of 8."""
    vol, mask = volume("ragged"), mask_of("ragged", "verbatim")
    part, mpart = np.ascontiguousarray(vol[:16, :16, :32]), np.ascontiguousarray(mask[:16, :16, :32])
    codec = BlockBoundedCodec(16, 0)
    blob = codec.encode(part, mask=mpart)
    assert blob == expected(("ragged", RAGGED[1], 16, 0, "verbatim"))[1][0]
    dec = codec.decode(blob).reshape(part.shape)
    np.testing.assert_array_equal(dec, ref.decode_chunk(blob))
    assert np.all(np.abs(dec.astype(np.int64) - part) <= np.where(mpart != 0, 0, 16))
    edge = np.ascontiguousarray(vol[16:, 16:, 32:])                    # (4, 1, 8) -> nominal (8, 8, 8)
    blob = BlockBoundedCodec(1).encode(edge)
    want, rec, _ = ref.encode_chunk(edge, (8, 8, 8), ref.bounds(edge.shape, 1))
    assert blob == want
    np.testing.assert_array_equal(BlockBoundedCodec(1).decode(blob).reshape(edge.shape), rec)


# ---- buffers ---------------------------------------------------------------------------------------------------------
BUFFER_CASE = ("ragged", RAGGED[1], 16, 0, "verbatim")


def guards_intact(view, what):
    got = view._download()
    np.testing.assert_array_equal(got[:view.lo], view.host[:view.lo], err_msg=f"{what}: bytes before the view")
    np.testing.assert_array_equal(got[view.hi:], view.host[view.hi:], err_msg=f"{what}: bytes after the view")


@pytest.mark.parametrize("fill", [0xA5, 0x00])
def test_encode_and_decode_on_poisoned_guarded_buffers(ctx, oracle, fill):
    """out_capacity is the bound exactly and the container starts 16 bytes into a poisoned buffer: streams and pads
    equal the restatement's, nothing around out, sizes, offsets or the decoded volume is written, inputs stay as they
    were, and a capacity one byte short is refused with everything untouched."""
    name, chunk, delta, delta_fg, kind = BUFFER_CASE
    vol, mask = volume(name), mask_of(name, kind)
    want, _, rec, _ = expected(BUFFER_CASE)
    data, offsets, sizes = want
    shape = vol.shape
    cap = _native.block_bounded_volume_bound(shape, chunk)
    assert data.size <= cap
    what = f"block-bounded {shape}/{chunk} fill {fill:#x}"
    with Views(ctx, fill) as view:
        v_in, v_mask = view(np.uint16, vol.size, 1, vol), view(np.uint8, mask.size, 3, mask)
        v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, offsets.size, 1)
        v_sz = view(np.uint32, sizes.size, 3)
        with pytest.raises(ValueError, match="out_capacity is below"):
            ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr, out=v_out.ptr,
                                     out_capacity=cap - 1, offsets=v_off.ptr, sizes=v_sz.ptr)
        ctx.sync()
        for v in (v_in, v_mask, v_out, v_off, v_sz):
            v.check_untouched(f"{what}: refused encode")
        totals = ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr, out=v_out.ptr,
                                          out_capacity=cap, offsets=v_off.ptr, sizes=v_sz.ptr)
        check_container(v_out, v_off, v_sz, totals, want, what)
        v_sz2 = view(np.uint32, sizes.size, 1)
        assert ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr,
                                        sizes=v_sz2.ptr) == totals
        v_sz2.check_output(sizes, f"{what}: sizes only")
        v_in.check_untouched(f"{what}: vol")
        v_mask.check_untouched(f"{what}: mask")
        # in_bytes is the container length exactly: the fill, not zeros, lies behind it
        v_cont, v_offin = view(np.uint8, data.size, OUT_K, data), view(np.uint64, offsets.size, 1, offsets)
        v_dec = view(np.uint16, vol.size, 3)
        ctx.block_bounded_decode(v_cont.ptr, data.size, v_offin.ptr, shape, chunk, v_dec.ptr)
        v_dec.check_output(rec, f"{what}: decoded vol")
        v_cont.check_untouched(f"{what}: in")
        v_offin.check_untouched(f"{what}: offsets_dev of the decoder")


def _corruptions():
    """Containers of the buffer case with one defect each, made from the restatement's streams."""
    (data, offsets, sizes), _, _, planes = expected(BUFFER_CASE)
    k = next(i for i, p in enumerate(planes) if p is not None and (p == -2).any() and (p >= 0).any())
    at = int(offsets[k]) + 32
    inside, outside = int(np.nonzero(planes[k] >= 0)[0][0]), int(np.nonzero(planes[k] == -2)[0][0])
    step29, stepped = data.copy(), data.copy()
    step29[at + inside] = 29
    stepped[at + outside] = 12
    beyond = offsets.copy()
    beyond[-1] += 16
    return {"plane byte 29": (step29, offsets), "outside block with a step": (stepped, offsets),
            "last offset beyond in_bytes": (data, beyond)}


@pytest.mark.parametrize("defect", ["plane byte 29", "outside block with a step", "last offset beyond in_bytes"])
def test_malformed_containers_are_refused_on_the_device(ctx, oracle, defect):
    """EXABM4D_ERR_INVALID (ValueError) with nothing written around the output volume and the inputs as they were;
    the good container decodes right after."""
    name, chunk = BUFFER_CASE[0], BUFFER_CASE[1]
    vol = volume(name)
    (good, offsets, _), _, rec, _ = expected(BUFFER_CASE)
    data, offs = _corruptions()[defect]
    with Views(ctx, 0xA5) as view:
        v_cont, v_off = view(np.uint8, data.size, OUT_K, data), view(np.uint64, offs.size, 0, offs)
        v_dec = view(np.uint16, vol.size, 1)
        with pytest.raises(ValueError, match="malformed chunk stream"):
            ctx.block_bounded_decode(v_cont.ptr, data.size, v_off.ptr, vol.shape, chunk, v_dec.ptr)
        guards_intact(v_dec, defect)
        v_cont.check_untouched(f"{defect}: in")
        v_off.check_untouched(f"{defect}: offsets_dev")
        v_good, v_goff = view(np.uint8, good.size, OUT_K, good), view(np.uint64, offsets.size, 0, offsets)
        ctx.block_bounded_decode(v_good.ptr, good.size, v_goff.ptr, vol.shape, chunk, v_dec.ptr)
        v_dec.check_output(rec, f"{defect}: decode after the refusal")


# ---- chunk store -----------------------------------------------------------------------------------------------------
def test_zarr_round_trip(oracle, tmp_path):
    name, chunk, delta, delta_fg, kind = BUFFER_CASE
    vol, mask = volume(name), mask_of(name, kind)
    _, streams, rec, _ = expected(BUFFER_CASE)
    path = str(tmp_path / "store")
    ratio = chunk_store.write_zarr(vol, path, chunks=(1, 1) + chunk, codec=BlockBoundedCodec(delta, delta_fg),
                                   mask=mask)
    assert ratio == vol.nbytes / sum(len(s) for s in streams)
    enc, meta = chunk_store.read_encoded(path)
    assert meta["codecs"] == [{"name": "exac-dctq-block",
                               "configuration": {"version": 1, "max_error": delta, "fg_max_error": delta_fg,
                                                 "edge_chunks": "truncated"}}]
    assert [enc.chunk_bytes(i) for i in range(len(streams))] == streams
    back = chunk_store.read_zarr(path)                                  # the decoder comes from zarr.json
    assert back.shape == (1, 1) + vol.shape
    np.testing.assert_array_equal(back[0, 0], rec)
    with pytest.raises(ValueError):
        chunk_store.write_zarr(vol, str(tmp_path / "other"), chunks=(1, 1) + chunk, mask=mask)


def test_read_chunk_round_trip(oracle, tmp_path):
    name, chunk, delta, delta_fg, kind = BUFFER_CASE
    vol, mask = volume(name), mask_of(name, kind)
    rec = expected(BUFFER_CASE)[2]
    path = str(tmp_path / "store")
    chunk_store.write_zarr(vol, path, chunks=(1, 1) + chunk, codec=BlockBoundedCodec(delta, delta_fg), mask=mask)
    for key in ((0, 0, 0), (1, 1, 1)):                                  # a mode-1 chunk with verbatim blocks, an edge
        s = tuple(slice(i * c, min((i + 1) * c, n)) for i, c, n in zip(key, chunk, vol.shape))
        got = chunk_store.read_chunk(path, *key)
        assert got.shape == vol[s].shape
        np.testing.assert_array_equal(got, rec[s])
