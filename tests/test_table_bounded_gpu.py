"""Block-bounded codec with a bound table on the MI355X against tests/table_bounded_pyref.py: streams
byte for byte, the step planes, the decode voxel for voxel, and the guarantee
|decoded - input| <= min(T[input], where(mask, fg_max_error, max_error)) checked directly.  All comparisons are
equalities."""
import numpy as np
import pytest

import table_bounded_pyref as ref
from test_codec_buffers_gpu import OUT_K, Views, check_container, layout_container

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.noise import bound_table

pytestmark = pytest.mark.gpu

MAIN_SHAPE, MAIN_CHUNK = ref.MAIN
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
        if name == "main":
            return _frozen(ref.pg_volume(MAIN_SHAPE))
        if name == "voxel":
            return _frozen(np.full((1, 1, 1), 4242, np.uint16))
        if name == "constant":
            return _frozen(np.full((9, 9, 9), 1000, np.uint16))
        assert name == "chunk64"
        return _frozen(ref.pg_volume((64, 64, 64), seed=3))
    return cached(("vol", name), make)


def table(kind):
    def make():
        if kind in ("k0.5", "k2"):
            return _frozen(bound_table(ref.NOISE, float(kind[1:])))
        if kind == "random32":                  # non-monotone: every voxel has to look up its own value
            return _frozen(np.random.default_rng(7).integers(0, 33, 65536).astype(np.uint16))
        return _frozen(np.full(65536, {"zero": 0, "four": 4}[kind], np.uint16))
    return cached(("table", kind), make)


def mask_of(name, kind):
    """None, a random 10 %, or the voxels of every block the restatement finds verbatim at a bound of 0 (with
    fg_max_error = 0 those blocks stay verbatim inside chunks that are otherwise coded under the table)."""
    if kind is None:
        return None

    def make():
        vol = volume(name)
        if kind == "random10":
            return _frozen((np.random.default_rng(5).random(vol.shape) < 0.1).astype(np.uint8))
        assert name == "main" and kind == "verbatim"
        m = np.zeros(vol.shape, np.uint8)
        for st, s in zip(ref.volume_steps(vol, MAIN_CHUNK, 0), ref.chunk_slices(vol.shape, MAIN_CHUNK)):
            for bz, by, bx in zip(*np.nonzero(st == -1)):
                z0, y0, x0 = s[0].start + 8 * bz, s[1].start + 8 * by, s[2].start + 8 * bx
                m[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = 1
        assert m.any()
        return _frozen(m)
    return cached(("mask", name, kind), make)


#        volume      chunk           max_error  fg_max_error  mask        table
CASES = [("main", MAIN_CHUNK, 65535, None, None, "k0.5"),
         ("main", MAIN_CHUNK, 65535, None, None, "k2"),
         ("main", MAIN_CHUNK, 65535, 0, "random10", "k0.5"),
         ("main", MAIN_CHUNK, 65535, 0, "random10", "k2"),
         ("main", MAIN_CHUNK, 8, 1, "random10", "k0.5"),
         ("main", MAIN_CHUNK, 8, 1, "random10", "k2"),
         ("main", MAIN_CHUNK, 65535, 0, "verbatim", "k2"),
         ("main", MAIN_CHUNK, 65535, None, None, "random32"),
         ("main", MAIN_CHUNK, 65535, None, None, "zero"),
         ("main", MAIN_CHUNK, 65535, None, None, "four"),
         ("voxel", (8, 8, 8), 65535, None, None, "k2"),
         ("constant", (16, 16, 16), 65535, None, None, "k0.5"),
         ("chunk64", (64, 64, 64), 65535, None, None, "k2")]
IDS = ["-".join(str(v) for v in (c[0],) + c[2:]) for c in CASES]


def expected(case):
    """-> ((container, offsets, sizes), streams, reconstruction, step planes, steps of every chunk) of the
    restatement, computed once."""
    name, chunk, delta, delta_fg, mkind, tkind = case

    def make():
        vol, mask, tab = volume(name), mask_of(name, mkind), table(tkind)
        streams, rec, planes = ref.encode_volume(vol, chunk, delta, delta_fg, mask, tab)
        steps = np.stack(ref.volume_steps(vol, chunk, delta, delta_fg, mask, tab))
        return layout_container(streams), streams, _frozen(rec), planes, _frozen(steps)
    return cached(("enc",) + case, make)


def bound_of(case):
    name, _, delta, delta_fg, mkind, tkind = case
    vol, m = volume(name), mask_of(name, mkind)
    b = np.full(vol.shape, delta) if m is None else np.where(m != 0, delta_fg, delta)
    return np.minimum(table(tkind)[vol].astype(np.int64), b)


def codec_of(case):
    return BlockBoundedCodec(case[2], case[3], bound_table=table(case[5]))


def test_the_cases_reach_every_kind_of_chunk_and_block(oracle):
    """From the restatement's output alone: chunks of either mode, verbatim and outside blocks, many steps; and with
    the k = 2 table the step varies over the inside blocks of the main volume, so that a kernel which ignored the
    table could not pass where the table is merely slack (max_error is 65535 there: without the table every inside
    block would take the coarsest step)."""
    modes0 = modes1 = verbatim = outside = 0
    steps = set()
    for case in CASES:
        for p in expected(case)[3]:
            if p is None:
                modes0 += 1
                continue
            modes1 += 1
            verbatim += int((p == -1).sum())
            outside += int((p == -2).sum())
            steps |= set(p[p >= 0].tolist())
    assert min(modes0, modes1, verbatim, outside) >= 1 and len(steps) >= 8, (modes0, modes1, verbatim, outside, steps)
    st = expected(CASES[1])[4]
    assert len(set(st[st >= 0].tolist())) >= 4
    loose = np.stack(ref.volume_steps(volume("main"), MAIN_CHUNK, 65535))
    assert set(loose[loose != -2].tolist()) == {ref.base.STEPS - 1}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_streams_steps_and_decode_equal_the_restatement(oracle, case):
    name, chunk, delta, delta_fg, mkind, tkind = case
    vol, mask = volume(name), mask_of(name, mkind)
    (data, offsets, sizes), streams, rec, planes, steps = expected(case)
    codec = codec_of(case)
    enc = codec.encode_volume(vol, chunk, mask=mask)
    assert len(enc.sizes) == len(streams)
    for i, s in enumerate(streams):
        assert enc.chunk_bytes(i) == s, f"chunk {i}"
    np.testing.assert_array_equal(enc.offsets, offsets)
    np.testing.assert_array_equal(enc.data, data)                       # the padding between the streams too
    np.testing.assert_array_equal(codec.chunk_sizes(vol, chunk, mask=mask), sizes)     # out = NULL: sizes only
    got = BlockBoundedCodec.block_steps(enc)
    for a, b in zip(got, planes):
        assert (a is None and b is None) or np.array_equal(a, b)
    sel = codec.select_steps(vol, chunk, mask=mask)
    assert sel.dtype == np.int16 and sel.shape == ref.grid(vol.shape, chunk) + tuple(c // 8 for c in chunk)
    np.testing.assert_array_equal(sel.reshape(steps.shape), steps)
    dec = BlockBoundedCodec(delta, delta_fg).decode_volume(enc)        # the decoder has no table
    assert dec.dtype == np.uint16 and dec.shape == vol.shape
    np.testing.assert_array_equal(dec, rec)
    err = np.abs(dec.astype(np.int64) - vol.astype(np.int64))
    assert np.all(err <= bound_of(case)), f"largest excess {int((err - bound_of(case)).max())}"
    if tkind == "zero":
        np.testing.assert_array_equal(dec, vol)


def test_the_step_follows_the_intensity(oracle):
    """bound_table(k = 2) under max_error = 65535: the device's step plane is not constant over the inside blocks of
    the main volume (the restatement's is not either: test_the_cases_reach_...)."""
    case = CASES[1]
    want = expected(case)[4]
    assert len(set(want[want >= 0].tolist())) >= 4
    sel = codec_of(case).select_steps(volume("main"), MAIN_CHUNK)
    inside = sel[sel != -2]
    assert inside.size == int((want != -2).sum()) and len(set(inside.tolist())) >= 4


def test_constant_table_gives_the_bytes_of_the_entry_without_a_table(oracle):
    """T == 4 under max_error = 65535 against ``exabm4d_block_bounded_encode_dev`` at max_error = 4, and T == 65535
    (which binds nowhere) under (8, 1) with the mask against the table-less entry at (8, 1)."""
    vol, mask = volume("main"), mask_of("main", "random10")
    plain = BlockBoundedCodec(4).encode_volume(vol, MAIN_CHUNK)
    tab = BlockBoundedCodec(65535, bound_table=table("four")).encode_volume(vol, MAIN_CHUNK)
    np.testing.assert_array_equal(tab.data, plain.data)
    np.testing.assert_array_equal(tab.sizes, plain.sizes)
    np.testing.assert_array_equal(tab.offsets, plain.offsets)
    assert plain.data.tobytes() == expected(CASES[9])[0][0].tobytes()
    np.testing.assert_array_equal(BlockBoundedCodec(65535, bound_table=table("four")).select_steps(vol, MAIN_CHUNK),
                                  BlockBoundedCodec(4).select_steps(vol, MAIN_CHUNK))
    slack = np.full(65536, 65535, np.uint16)
    plain = BlockBoundedCodec(8, 1).encode_volume(vol, MAIN_CHUNK, mask=mask)
    tab = BlockBoundedCodec(8, 1, bound_table=slack).encode_volume(vol, MAIN_CHUNK, mask=mask)
    np.testing.assert_array_equal(tab.data, plain.data)
    np.testing.assert_array_equal(tab.sizes, plain.sizes)


# ---- buffers ---------------------------------------------------------------------------------------------------------
BUFFER_CASE = CASES[5]                          # main volume, (8, 1) with the mask, k = 2


@pytest.mark.parametrize("fill", [0xA5, 0x00])
def test_table_at_an_odd_element_of_a_poisoned_buffer(ctx, oracle, fill):
    """The table sits one element (2 bytes: 2-byte aligned, not 4) into a poisoned, guarded buffer, as do the other
    arguments: container, offsets, sizes and the step planes equal the restatement's and the aligned run's, the
    sizes-only call (out = NULL) returns the same sizes and totals, nothing around any output is written, and the
    table, the volume and the mask come back as they were.  A table at an odd byte is refused with nothing written."""
    name, chunk, delta, delta_fg, mkind, tkind = BUFFER_CASE
    vol, mask, tab = volume(name), mask_of(name, mkind), table(tkind)
    want, _, _, _, steps = expected(BUFFER_CASE)
    data, offsets, sizes = want
    shape = vol.shape
    cap = _native.block_bounded_volume_bound(shape, chunk)
    nbp = ref.base.plane_bytes(chunk)
    what = f"table-bounded {shape}/{chunk} fill {fill:#x}"
    with Views(ctx, fill) as view:
        v_in, v_mask = view(np.uint16, vol.size, 1, vol), view(np.uint8, mask.size, 3, mask)
        v_odd, v_even = view(np.uint16, 65536, 1, tab), view(np.uint16, 65536, 0, tab)
        assert v_odd.ptr % 4 == 2 and v_even.ptr % 16 == 0
        results = []
        for v_tab in (v_odd, v_even):
            v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, offsets.size, 1)
            v_sz = view(np.uint32, sizes.size, 3)
            totals = ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr,
                                              out=v_out.ptr, out_capacity=cap, offsets=v_off.ptr, sizes=v_sz.ptr,
                                              table=v_tab.ptr)
            check_container(v_out, v_off, v_sz, totals, want, what)
            v_sz2 = view(np.uint32, sizes.size, 1)
            assert ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr,
                                            sizes=v_sz2.ptr, table=v_tab.ptr) == totals
            v_sz2.check_output(sizes, f"{what}: sizes only")
            v_plane = view(np.uint8, steps.shape[0] * nbp, 0)
            ctx.block_bounded_steps(v_in.ptr, shape, chunk, delta, delta_fg, v_plane.ptr, mask=v_mask.ptr,
                                    table=v_tab.ptr)
            ctx.sync()
            plane = v_plane._download()[v_plane.lo:v_plane.hi].reshape(steps.shape[0], nbp)
            v_plane.check_output(plane, f"{what}: step planes")
            results.append(plane)
            st = plane[:, :steps[0].size].astype(np.int16)
            st[st == 0xFE] = -1
            st[st == 0xFF] = -2
            np.testing.assert_array_equal(st.reshape(steps.shape), steps)
            assert not plane[:, steps[0].size:].any()
        np.testing.assert_array_equal(results[0], results[1])
        # refused before anything is launched: outputs keep their fill
        v_out, v_off = view(np.uint8, cap, OUT_K), view(np.uint64, offsets.size, 1)
        v_sz, v_plane = view(np.uint32, sizes.size, 3), view(np.uint8, steps.shape[0] * nbp, 0)
        with pytest.raises(ValueError, match="bound_table"):
            ctx.block_bounded_encode(v_in.ptr, shape, chunk, delta, delta_fg, mask=v_mask.ptr, out=v_out.ptr,
                                     out_capacity=cap, offsets=v_off.ptr, sizes=v_sz.ptr, table=v_even.ptr + 1)
        with pytest.raises(ValueError, match="bound_table"):
            ctx.block_bounded_steps(v_in.ptr, shape, chunk, delta, delta_fg, v_plane.ptr, mask=v_mask.ptr,
                                    table=v_even.ptr + 1)
        ctx.sync()
        for v in (v_out, v_off, v_sz, v_plane, v_in, v_mask, v_odd, v_even):
            v.check_untouched(f"{what}: inputs, and the outputs of the refused calls")


# ---- chunk store -----------------------------------------------------------------------------------------------------
def test_through_the_store(oracle, tmp_path):
    """write_zarr with a codec from measured-style noise parameters, read_zarr with no codec argument: the decoder is
    picked from zarr.json, which has no table, and the volume comes back within the bound."""
    vol, mask = volume("main"), mask_of("main", "random10")
    tab = table("k0.5")
    streams, rec, _ = ref.encode_volume(vol, MAIN_CHUNK, 65535, None, mask, tab)
    path = str(tmp_path / "store")
    codec = BlockBoundedCodec.from_noise(ref.NOISE, 0.5)
    np.testing.assert_array_equal(codec.bound_table, tab)
    ratio = chunk_store.write_zarr(vol, path, chunks=(1, 1) + MAIN_CHUNK, codec=codec, mask=mask)
    assert ratio == vol.nbytes / sum(len(s) for s in streams)
    enc, meta = chunk_store.read_encoded(path)
    assert meta["codecs"] == [{"name": "exac-dctq-block",
                               "configuration": {"version": 1, "max_error": 65535, "fg_max_error": 65535,
                                                 "edge_chunks": "truncated",
                                                 "bound": {"kind": "poisson-gaussian", "gain": 2.0,
                                                           "read_noise": 3.0, "offset": 100.0, "k": 0.5}}}]
    assert [enc.chunk_bytes(i) for i in range(len(streams))] == streams
    back = chunk_store.read_zarr(path)
    assert back.shape == (1, 1) + vol.shape
    np.testing.assert_array_equal(back[0, 0], rec)
    assert np.all(np.abs(back[0, 0].astype(np.int64) - vol) <= tab[vol])
    got = chunk_store.read_chunk(path, 1, 1, 1)                         # an edge chunk, alone
    np.testing.assert_array_equal(got, rec[16:, 16:, 24:])
