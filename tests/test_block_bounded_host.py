"""Error-bounded codec with a step per 8^3 block (format "EB" version 1), host side: the 32-byte
header, everything a stream is checked for before any device call, the restatement's own guarantee, the chunk
store's exac-dctq-block metadata, and the rate against the per-chunk format.  No GPU."""
import json
import os
import struct

import numpy as np
import pytest

import block_bounded_pyref as ref
import bounded_pyref as chunk_ref
from util import synth_volume

from aind_exaspim_image_compression.utils import block_bounded_codec as B
from aind_exaspim_image_compression.utils import chunk_store


@pytest.mark.parametrize("mode,extent,chunk", [(0, (64, 64, 64), (64, 64, 64)), (1, (1, 1, 1), (8, 8, 8)),
                                               (1, (7, 8, 9), (8, 8, 16)), (1, (40, 64, 48), (64, 64, 48)),
                                               (0, (100, 3, 8), (104, 8, 8))])
def test_header_round_trip(mode, extent, chunk):
    h = B.pack_header(mode, extent, chunk)
    assert len(h) == 32 and h == ref.header(mode, extent, chunk)
    assert h[:4] == b"EB" + bytes((1, mode)) and h[4:12] == bytes(8) and h[24:32] == bytes(8)
    assert struct.unpack("<6H", h[12:24]) == extent + chunk
    nb = (chunk[0] // 8) * (chunk[1] // 8) * (chunk[2] // 8)
    assert B.plane_bytes(chunk) == ref.plane_bytes(chunk) == -(-nb // 16) * 16
    if mode == 1:
        inside = B._inside_blocks(extent, chunk)
        plane = np.zeros(B.plane_bytes(chunk), np.uint8)
        plane[:nb] = np.where(inside, 7, 0xFF)
        plane[0] = 0xFE
        exac = b"EX\x02\x04" + struct.pack("<3I", nb * 512, 8, 64)
        got = B.parse_header(h + plane.tobytes() + exac)
        want = np.where(inside, 7, -2)
        want[0] = -1
        assert got["steps"].dtype == np.int16
        np.testing.assert_array_equal(got["steps"], want)
    else:
        exac = b"EX\x02\x02" + struct.pack("<3I", extent[0] * extent[1] * extent[2], extent[1], extent[2])
        got = B.parse_header(h + exac)
        assert got["steps"] is None
    assert got["mode"] == mode and got["extent"] == extent and got["chunk"] == chunk


def _mutate(h, at, value):
    b = bytearray(h)
    b[at:at + len(value)] = value
    return bytes(b)


# (8, 16, 20) in (16, 16, 24): nominal grid (2, 2, 3) = 12 blocks in a plane of 16 bytes; the six blocks of z = 0 are
# inside, blocks 6..11 outside
_EXTENT, _CHUNK = (8, 16, 20), (16, 16, 24)
_PLANE = bytes([5, 28, 0xFE, 0, 12, 12] + [0xFF] * 6 + [0] * 4)
GOOD = B.pack_header(1, _EXTENT, _CHUNK) + _PLANE + b"EX\x02\x04" + struct.pack("<3I", 12 * 512, 8, 64) + bytes(16)
GOOD0 = B.pack_header(0, _EXTENT, _CHUNK) + b"EX\x02\x02" + struct.pack("<3I", 8 * 16 * 20, 16, 20) + bytes(16)
BAD = {
    "magic": _mutate(GOOD, 0, b"EQ"),
    "version": _mutate(GOOD, 2, b"\x02"),
    "mode": _mutate(GOOD, 3, b"\x02"),
    "reserved_front": _mutate(GOOD, 4, b"\x05"),
    "reserved_front_last": _mutate(GOOD, 11, b"\x01"),
    "reserved_back": _mutate(GOOD, 24, b"\x01"),
    "reserved_back_last": _mutate(GOOD0, 31, b"\x80"),
    "extent_beyond_chunk": _mutate(GOOD, 12, struct.pack("<H", 17)),
    "extent_zero": _mutate(GOOD, 14, struct.pack("<H", 0)),
    "chunk_not_multiple_of_8": _mutate(GOOD, 22, struct.pack("<H", 20)),
    "chunk_zero": _mutate(_mutate(GOOD, 18, struct.pack("<H", 0)), 12, struct.pack("<H", 0)),
    "plane_byte_29": _mutate(GOOD, 32 + 1, b"\x1d"),
    "outside_marker_on_inside_block": _mutate(GOOD, 32 + 4, b"\xff"),
    "step_on_outside_block": _mutate(GOOD, 32 + 7, b"\x0c"),
    "verbatim_on_outside_block": _mutate(GOOD, 32 + 11, b"\xfe"),
    "plane_padding": _mutate(GOOD, 32 + 12, b"\x01"),
    "plane_padding_last": _mutate(GOOD, 32 + 15, b"\xff"),
    "payload_typesize": _mutate(GOOD, 48 + 3, b"\x02"),
    "payload_count": _mutate(GOOD, 48 + 4, struct.pack("<I", 11 * 512)),
    "payload_not_exac": _mutate(GOOD, 48, b"EQ"),
    "lossless_payload_rows": _mutate(GOOD0, 32 + 8, struct.pack("<I", 20)),
    "lossless_as_blocks": _mutate(GOOD0, 3, b"\x01"),
    "truncated_header": GOOD[:20],
    "header_only": GOOD[:32],
    "truncated_plane": GOOD[:40],
    "truncated_payload": GOOD[:48 + 8],
    "empty": b"",
}


def test_good_streams_parse():
    np.testing.assert_array_equal(B.parse_header(GOOD)["steps"], [5, 28, -1, 0, 12, 12] + [-2] * 6)
    assert B.parse_header(GOOD0)["mode"] == 0


@pytest.mark.parametrize("case", sorted(BAD))
def test_malformed_stream_raises_on_the_host(case, monkeypatch):
    # any device call would go through _native.context: make it fail loudly if it is reached
    from aind_exaspim_image_compression import _native

    def no_device(*a, **k):
        raise AssertionError("a malformed stream reached the device")

    monkeypatch.setattr(_native, "context", no_device)
    with pytest.raises(ValueError):
        B.parse_header(BAD[case])
    with pytest.raises(ValueError):
        B.BlockBoundedCodec(4).decode(BAD[case])


def test_codec_arguments():
    c = B.BlockBoundedCodec(7)
    assert c.codec_id == "exac-dctq-block" and c.version == 1 and (c.max_error, c.fg_max_error) == (7, 7)
    assert c.get_config() == {"id": "exac-dctq-block", "max_error": 7, "fg_max_error": 7, "version": 1}
    c = B.BlockBoundedCodec(7, 0)
    assert (c.max_error, c.fg_max_error) == (7, 0)
    assert B.BlockBoundedCodec(65535, 65535).fg_max_error == 65535
    for bad in ((-1, None), (65536, None), (4, 5), (4, -1), (65536, 0)):
        with pytest.raises(ValueError):
            B.BlockBoundedCodec(*bad)


def test_mask_of_another_shape_is_refused(monkeypatch):
    from aind_exaspim_image_compression import _native

    def no_device(*a, **k):
        raise AssertionError("a mask of the wrong shape reached the device")

    monkeypatch.setattr(_native, "context", no_device)
    vol = np.zeros((8, 8, 16), np.uint16)
    for shape in ((8, 8, 8), (8, 16, 8), (8, 8, 16, 2), (1024,)):
        with pytest.raises(ValueError):
            B.BlockBoundedCodec(4, 0).encode_volume(vol, (8, 8, 8), mask=np.zeros(shape, np.uint8))
        with pytest.raises(ValueError):
            B.BlockBoundedCodec(4, 0).chunk_sizes(vol, (8, 8, 8), mask=np.zeros(shape, bool))


@pytest.fixture(scope="module")
def masked_case(oracle):
    """A ragged volume with a mask that covers a bright structure and a few lone voxels."""
    shape, chunk = (20, 17, 30), (16, 8, 24)
    vol, clean = synth_volume(shape, seed=3, sigma=3.0, as_u16=True)
    mask = (clean > 60).astype(np.uint8)
    mask[0, 0, 0] = mask[19, 16, 29] = mask[8, 8, 24] = 1
    assert 0 < mask.sum() < mask.size
    return shape, chunk, vol, mask


@pytest.mark.parametrize("delta,delta_fg", [(0, 0), (4, 4), (4, 0), (8, 1), (16, 0), (65535, 0)])
def test_restatement_keeps_the_bound_on_masked_input(masked_case, delta, delta_fg):
    shape, chunk, vol, mask = masked_case
    b = np.where(mask != 0, delta_fg, delta)
    streams, rec, planes = ref.encode_volume(vol, chunk, delta, delta_fg, mask)
    assert len(streams) == int(np.prod(ref.grid(shape, chunk)))
    assert np.all(np.abs(rec.astype(np.int64) - vol) <= b)
    for s, blob, plane in zip(ref.chunk_slices(shape, chunk), streams, planes):
        d = ref.decode_chunk(blob)
        np.testing.assert_array_equal(d, rec[s])
        assert np.all(np.abs(d.astype(np.int64) - vol[s]) <= b[s])
        h = B.parse_header(blob)
        assert h["extent"] == vol[s].shape and h["chunk"] == chunk
        if plane is None:
            assert h["mode"] == 0 and h["steps"] is None
            np.testing.assert_array_equal(d, vol[s])
        else:
            assert h["mode"] == 1
            np.testing.assert_array_equal(h["steps"], plane)
    if delta == 0:
        np.testing.assert_array_equal(rec, vol)


def test_store_metadata_is_read_back(masked_case, tmp_path):
    """A store assembled from the restatement's chunk streams and the exac-dctq-block metadata reads back as the same
    container (host only: the oracle codes the chunks)."""
    shape, chunk, vol, mask = masked_case
    streams, _, planes = ref.encode_volume(vol, chunk, 8, 1, mask)
    codec = B.BlockBoundedCodec(8, 1)
    meta = chunk_store.metadata(shape, chunk, codec=codec)
    assert meta["data_type"] == "uint16"
    assert meta["codecs"] == [{"name": "exac-dctq-block",
                               "configuration": {"version": 1, "max_error": 8, "fg_max_error": 1,
                                                 "edge_chunks": "truncated"}}]
    path = str(tmp_path / "store")
    g = ref.grid(shape, chunk)
    k = 0
    for iz in range(g[0]):
        for iy in range(g[1]):
            for ix in range(g[2]):
                p = os.path.join(path, chunk_store.chunk_key(iz, iy, ix))
                os.makedirs(os.path.dirname(p), exist_ok=True)
                with open(p, "wb") as f:
                    f.write(streams[k])
                k += 1
    with open(os.path.join(path, "zarr.json"), "w") as f:
        json.dump(meta, f)
    enc, meta2 = chunk_store.read_encoded(path)
    assert meta2["codecs"][0]["name"] == "exac-dctq-block"
    assert enc.shape == shape and enc.chunk == chunk and enc.typesize == 2
    assert [enc.chunk_bytes(i) for i in range(len(streams))] == streams
    assert np.all(enc.offsets % 16 == 0)
    picked = chunk_store._codec_of(meta2)
    assert isinstance(picked, B.BlockBoundedCodec) and (picked.max_error, picked.fg_max_error) == (8, 1)
    got = B.BlockBoundedCodec.block_steps(enc)
    assert len(got) == len(planes)
    for a, b in zip(got, planes):
        assert (a is None and b is None) or np.array_equal(a, b)
    # write_encoded writes the same entry
    path2 = str(tmp_path / "store2")
    chunk_store.write_encoded(enc, path2, codec=codec)
    with open(os.path.join(path2, "zarr.json")) as f:
        assert json.load(f)["codecs"] == meta["codecs"]
    enc2, _ = chunk_store.read_encoded(path2)
    np.testing.assert_array_equal(enc2.data, enc.data)
    # a wrong configuration is refused like every other unsupported store
    for key, value in (("version", 2), ("fg_max_error", 9), ("max_error", 65536)):
        bad = json.loads(json.dumps(meta))
        bad["codecs"][0]["configuration"][key] = value
        with open(os.path.join(path, "zarr.json"), "w") as f:
            json.dump(bad, f)
        with pytest.raises(ValueError):
            chunk_store.read_encoded(path)
    bad = json.loads(json.dumps(meta))
    del bad["codecs"][0]["configuration"]["fg_max_error"]
    with open(os.path.join(path, "zarr.json"), "w") as f:
        json.dump(bad, f)
    with pytest.raises(ValueError):
        chunk_store.read_encoded(path)


def test_a_step_per_block_is_smaller_than_a_step_per_chunk(oracle):
    """64^3 chunks of a synthetic volume with bright structures: the restatement's container, step planes included,
    against the per-chunk restatement's at the same bound.  Integer results of numpy's seeded generator."""
    shape, chunk = (64, 64, 128), (64, 64, 64)
    vol, _ = synth_volume(shape, seed=5, sigma=3.0, as_u16=True)
    errs = chunk_ref.volume_ladder(vol, chunk)
    for delta in (2, 8):
        block = sum(len(s) for s in ref.encode_volume(vol, chunk, delta)[0])
        per_chunk = sum(len(s) for s in chunk_ref.encode_volume(vol, chunk, delta, errs)[0])
        print(f"max_error {delta}: {block} bytes per block, {per_chunk} per chunk")
        assert block < per_chunk
