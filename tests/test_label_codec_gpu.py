"""The label codec ``exac-labels`` on the MI355X (csrc/label_codec_kernels.hip through ``LabelCodec`` and
``_native.Context``) against the numpy restatement tests/label_pyref.py: bytes chunk for chunk, round trips, the bound,
guarded buffers, and a palette index past its palette.  Integer data: every comparison is exact."""
import struct

import numpy as np
import pytest

import label_pyref as ref
from util import GuardedView

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume
from aind_exaspim_image_compression.utils.label_codec import LabelCodec

pytestmark = pytest.mark.gpu

DTYPES = (np.uint32, np.uint64)
# name -> (volume, chunk): truncated chunks and blocks on every axis; a chunk that is no multiple of 8; one 64^3
# chunk of tubes and blobs; nothing but background
CASES = {
    "classes": (lambda dt: ref.class_volume((40, 24, 19), dt), (16, 16, 16)),
    "classes_odd_chunk": (lambda dt: ref.class_volume((40, 24, 19), dt), (20, 16, 24)),
    "tubes": (lambda dt: ref.tube_volume((64, 64, 64), dt), (64, 64, 64)),
    "zeros": (lambda dt: np.zeros((40, 24, 19), dt), (16, 16, 16)),
}
_cache = {}


def case(name, dtype):
    """(volume, clamped chunk, the pyref's stream of every chunk in raster order), computed once."""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        make, chunk = CASES[name]
        vol = make(dtype)
        chunk = tuple(min(c, s) for c, s in zip(chunk, vol.shape))
        grid = [-(-s // c) for s, c in zip(vol.shape, chunk)]
        blobs = [ref.encode(vol[iz * chunk[0]:(iz + 1) * chunk[0], iy * chunk[1]:(iy + 1) * chunk[1],
                                ix * chunk[2]:(ix + 1) * chunk[2]])
                 for iz in range(grid[0]) for iy in range(grid[1]) for ix in range(grid[2])]
        vol.setflags(write=False)
        _cache[key] = (vol, chunk, blobs)
    return _cache[key]


def container(blobs, shape, chunk, typesize):
    data, offsets, sizes = chunk_store.pack_streams(blobs)
    return EncodedVolume(data, offsets, sizes, shape, chunk, typesize)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_equal_the_pyref_and_round_trip(ctx, name, dtype):
    vol, chunk, blobs = case(name, dtype)
    codec = LabelCodec(vol.dtype.itemsize)
    enc = codec.encode_volume(vol, chunk=CASES[name][1])
    assert enc.chunk == chunk and enc.shape == vol.shape and len(enc.sizes) == len(blobs)
    for i, want in enumerate(blobs):
        got = enc.chunk_bytes(i)
        assert len(got) == len(want), (name, i)
        assert got == want, (name, i)
    assert enc.offsets.tolist() == np.concatenate(([0], np.cumsum((enc.sizes.astype(np.int64) + 15) // 16 * 16))).tolist()
    assert codec.chunk_sizes(vol, CASES[name][1]).tolist() == [len(b) for b in blobs]
    # the device's own bytes back, and the pyref's bytes through the device decoder
    assert np.array_equal(codec.decode_volume(enc), vol)
    back = codec.decode_volume(container(blobs, vol.shape, chunk, vol.dtype.itemsize))
    assert back.dtype == vol.dtype and np.array_equal(back, vol)
    # twice the same bytes, pads included; and from a buffer that is already on the device
    again = codec.encode_volume(vol, chunk=CASES[name][1])
    assert np.array_equal(again.data, enc.data) and np.array_equal(again.sizes, enc.sizes)
    with ctx.to_device(vol.reshape(-1)) as d_vol:
        dev = codec.encode_device(ctx, d_vol, vol.shape, CASES[name][1])
    assert np.array_equal(dev.data, enc.data) and np.array_equal(dev.offsets, enc.offsets)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_chunk_encode_and_decode(ctx, dtype):
    vol, chunk, blobs = case("classes", dtype)
    codec = LabelCodec(vol.dtype.itemsize)
    sub = np.ascontiguousarray(vol[32:40, 16:24, 16:19])            # the corner chunk: (8, 8, 3)
    blob = codec.encode(sub)
    assert blob == ref.encode(sub) == blobs[-1]
    assert np.array_equal(codec.decode(blob).reshape(sub.shape), sub)
    one = np.array([[[2 ** (8 * vol.dtype.itemsize) - 1]]], dtype=dtype)
    assert codec.encode(one) == ref.encode(one) and len(codec.encode(one)) == 48
    with pytest.raises(ValueError):
        codec.encode(sub.astype(np.uint16))
    with pytest.raises(ValueError):
        LabelCodec(12 - vol.dtype.itemsize).decode(blob)


def test_every_block_raw_stays_within_the_bound(ctx):
    rng = np.random.default_rng(11)
    shape, chunk = (24, 17, 33), (16, 16, 16)
    vol = rng.integers(0, 2 ** 63, shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    codec = LabelCodec(8)
    enc = codec.encode_volume(vol, chunk=chunk)
    bound = _native.label_encode_bound(8, shape, chunk)
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    i = 0
    for iz in range(grid[0]):
        for iy in range(grid[1]):
            for ix in range(grid[2]):
                sub = vol[iz * 16:(iz + 1) * 16, iy * 16:(iy + 1) * 16, ix * 16:(ix + 1) * 16]
                want = ref.encode(sub)
                assert enc.chunk_bytes(i) == want, (iz, iy, ix)
                i += 1
    # a condition on the input: every voxel differs, so every block of more than 256 voxels is raw
    assert np.all(ref.table(ref.encode(vol[:16, :16, :16]))[2] == 64)
    assert int(enc.offsets[-1]) <= bound and enc.nbytes <= bound
    assert np.array_equal(codec.decode_volume(enc), vol)
    # and a volume whose every block is full and raw meets the bound exactly
    cube = rng.integers(0, 2 ** 32, (16, 16, 16), dtype=np.uint32)
    enc = LabelCodec(4).encode_volume(cube, chunk=(16, 16, 16))
    if all(len(np.unique(cube[z:z + 8, y:y + 8, x:x + 8])) > 256 for z in (0, 8) for y in (0, 8) for x in (0, 8)):
        assert int(enc.offsets[-1]) == _native.label_encode_bound(4, (16, 16, 16), (16, 16, 16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["classes", "classes_odd_chunk"])
def test_guarded_buffers(ctx, name, dtype):
    """Encode into a container of exactly the bound between poisoned guards, decode into a poisoned view at an odd
    element offset (no 16-byte aligned row: the narrow stores): nothing but the streams, their pads and the volume
    is written."""
    vol, chunk, blobs = case(name, dtype)
    ts = vol.dtype.itemsize
    bound = _native.label_encode_bound(ts, vol.shape, chunk)
    data, offsets, sizes = chunk_store.pack_streams(blobs)
    v_in = GuardedView(ctx, vol.dtype, vol.size, k=1, data=vol)
    v_out = GuardedView(ctx, np.uint8, bound, k=16)
    v_off = GuardedView(ctx, np.uint64, len(blobs) + 1, k=1)
    v_sz = GuardedView(ctx, np.uint32, len(blobs), k=3)
    v_vol = GuardedView(ctx, vol.dtype, vol.size, k=3)
    try:
        total, held = ctx.label_encode(v_in.ptr, ts, vol.shape, chunk, out=v_out.ptr, out_capacity=bound,
                                       offsets=v_off.ptr, sizes=v_sz.ptr)
        assert (total, held) == (int(sizes.sum()), data.size) and held <= bound
        v_in.check_untouched("encode input")
        v_off.check_output(offsets, "offsets")
        v_sz.check_output(sizes, "sizes")
        want = np.full(bound, 0xA5, np.uint8)                       # the poison stays behind the container ...
        want[:data.size] = data
        assert all(-int(n) % 16 in (0, 8) for n in sizes)           # ... and a stream's pad to 16 bytes is zeroed
        v_out.check_output(want, "container")
        ctx.label_decode(v_out.ptr, held, v_off.ptr, ts, vol.shape, chunk, v_vol.ptr)
        v_vol.check_output(vol, "decoded volume")
        with pytest.raises(ValueError):                             # a capacity below the bound launches nothing
            ctx.label_encode(v_in.ptr, ts, vol.shape, chunk, out=v_out.ptr, out_capacity=bound - 1,
                             offsets=v_off.ptr, sizes=v_sz.ptr)
        v_off.check_output(offsets, "offsets after the refusal")
    finally:
        for v in (v_in, v_out, v_off, v_sz, v_vol):
            v.free()


def _patched(blob, at, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, *values)
    return bytes(b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_index_past_its_palette_is_clamped_and_reported(ctx, dtype):
    """Header and table valid, one index row of a 3-entry palette set to 3, 3, 3, 3: the kernel clamps the index to
    k - 1 before it reads the palette (lb_value in csrc/label_codec_kernels.hip), so the read stays inside the
    payload; the entry reports the stream and the guards around the output are as uploaded."""
    vol = ref.class_volume((16, 16, 11), dtype, counts=(1, 3, 17, 512))
    ts = vol.dtype.itemsize
    blob = ref.encode(vol)
    at, k, bits = ref.table(blob)
    b = int(np.flatnonzero((bits == 2) & (k == 3))[0])
    bz, by, bx = b // 4, b // 2 % 2, b % 2
    block = vol[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
    hurt = _patched(blob, 8 * int(at[b]) + (3 * ts + 7) // 8 * 8, "<B", 0xFF)       # row 0: slots 0..3 <- index 3
    want = vol.copy()
    want[8 * bz, 8 * by, 8 * bx:8 * bx + min(4, block.shape[2])] = np.unique(block)[2]
    codec = LabelCodec(ts)
    with pytest.raises(ValueError):
        codec.decode(hurt)
    data, offsets, sizes = chunk_store.pack_streams([hurt])
    v_vol = GuardedView(ctx, vol.dtype, vol.size, k=1)
    try:
        with ctx.to_device(data) as d_in, ctx.to_device(offsets) as d_off:
            with pytest.raises(ValueError, match="palette index"):
                ctx.label_decode(d_in, data.size, d_off, ts, vol.shape, vol.shape, v_vol.ptr)
            v_vol.check_output(want, "the clamped decode")
            # the context is usable afterwards, and the status is the call's own
            good = chunk_store.pack_streams([blob])
            with ctx.to_device(good[0]) as d_good:
                ctx.label_decode(d_good, good[0].size, d_off, ts, vol.shape, vol.shape, v_vol.ptr)
            v_vol.check_output(vol, "the next decode")
    finally:
        v_vol.free()


def test_a_table_entry_past_its_stream_decodes_to_zeros_and_is_reported(ctx):
    """What the host check exists to catch, handed to the entry without it: the last block of the first of two
    chunks points 64 bytes further, past its stream's total (but inside the container, where the second chunk lies).
    The kernel opens every block under its stream's bounds, so that block is zeros and the call raises."""
    vol = ref.class_volume((16, 16, 22), np.uint64, counts=(1, 3, 17, 512))
    chunk = (16, 16, 11)
    blobs = [ref.encode(vol[:, :, :11]), ref.encode(vol[:, :, 11:])]
    assert len(blobs[1]) > 64
    nblocks = struct.unpack_from("<I", blobs[0], 20)[0]
    at = ref.table(blobs[0])[0]
    hurt = _patched(blobs[0], ref.HEADER + 8 * (nblocks - 1), "<I", int(at[-1]) + 8)
    data, offsets, sizes = chunk_store.pack_streams([hurt, blobs[1]])
    want = vol.copy()
    want[8:16, 8:16, 8:11] = 0                                      # the last block of chunk 0
    v_vol = GuardedView(ctx, vol.dtype, vol.size, k=2)
    try:
        with ctx.to_device(data) as d_in, ctx.to_device(offsets) as d_off:
            with pytest.raises(ValueError, match="outside its bounds"):
                ctx.label_decode(d_in, data.size, d_off, 8, vol.shape, chunk, v_vol.ptr)
        v_vol.check_output(want, "decode of a rejected block")
    finally:
        v_vol.free()
    with pytest.raises(ValueError):                                 # and the host check refuses it before any of that
        LabelCodec(8).decode_volume(EncodedVolume(data, offsets, sizes, vol.shape, chunk, 8))


def test_entries_refuse_bad_arguments(ctx):
    with ctx.alloc(4096) as d:
        for shape, chunk, ts in (((8, 8, 8), (8, 8, 8), 2), ((0, 8, 8), (8, 8, 8), 8), ((8, 8, 8), (8, 0, 8), 4)):
            with pytest.raises(ValueError):
                ctx.label_encode(d, ts, shape, chunk)
            with pytest.raises(ValueError):
                _native.label_encode_bound(ts, shape, chunk)
        with pytest.raises(ValueError):
            ctx.label_encode(None, 8, (8, 8, 8), (8, 8, 8))
        with pytest.raises(ValueError):
            ctx.label_encode(d, 8, (8, 8, 8), (8, 8, 8), out=d, out_capacity=1 << 20)       # no offsets
        with pytest.raises(ValueError):
            ctx.label_decode(int(d.ptr) + 8, 64, d, 8, (8, 8, 8), (8, 8, 8), d)             # in not 16-byte aligned
