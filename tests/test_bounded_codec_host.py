"""Error-bounded lossy chunk codec, host side: the step ladder, the 32-byte chunk header and
its validation before any device call, and the chunk store's exac-dctq metadata.  No GPU."""
import json
import os
import struct

import numpy as np
import pytest

import bounded_pyref as ref

from aind_exaspim_image_compression.utils import bounded_codec as B
from aind_exaspim_image_compression.utils import chunk_store


def test_ladder_is_the_formula():
    want = np.array([np.float32(2.0 ** ((j - 4) / 4)) for j in range(29)], dtype=np.float32)
    assert B.LADDER.dtype == np.float32 and B.LADDER.shape == (29,)
    np.testing.assert_array_equal(B.LADDER, want)
    np.testing.assert_array_equal(B.LADDER, ref.LADDER)
    assert B.LADDER[0] == 0.5 and B.LADDER[4] == 1.0 and B.LADDER[28] == 64.0
    assert np.all(np.diff(B.LADDER) > 0)


@pytest.mark.parametrize("mode,j,extent,chunk", [(0, 0, (64, 64, 64), (64, 64, 64)), (1, 0, (1, 1, 1), (8, 8, 8)),
                                                 (1, 17, (7, 8, 9), (8, 8, 16)), (1, 28, (40, 64, 48), (64, 64, 48)),
                                                 (0, 5, (100, 3, 8), (104, 8, 8))])
def test_header_round_trip(mode, j, extent, chunk):
    h = B.pack_header(mode, j, extent, chunk)
    assert len(h) == 32 and h == ref.header(mode, j, extent, chunk)
    got = B.parse_header(h + b"\0")
    assert got["mode"] == mode and got["extent"] == extent and got["chunk"] == chunk
    if mode == 1:
        assert got["j"] == j and got["q"] == float(B.LADDER[j])
        assert struct.unpack("<f", h[8:12])[0] == B.LADDER[j]
    else:
        assert got["j"] is None and got["q"] == 0.0 and h[4] == 0xFF and h[8:12] == bytes(4)
    assert h[5:8] == bytes(3) and h[24:32] == bytes(8)


def _mutate(h, at, value):
    b = bytearray(h)
    b[at:at + len(value)] = value
    return bytes(b)


GOOD = B.pack_header(1, 9, (40, 64, 48), (64, 64, 48)) + bytes(16)
BAD = {
    "magic": _mutate(GOOD, 0, b"EX"),
    "version": _mutate(GOOD, 2, b"\x02"),
    "mode": _mutate(GOOD, 3, b"\x02"),
    "q_not_ladder": _mutate(GOOD, 8, struct.pack("<f", 3.0)),
    "q_other_step": _mutate(GOOD, 8, B.LADDER[10].tobytes()),
    "j_beyond_ladder": _mutate(GOOD, 4, b"\x1d"),
    "lossless_with_step": _mutate(GOOD, 3, b"\x00"),
    "extent_beyond_chunk": _mutate(GOOD, 12, struct.pack("<H", 65)),
    "extent_zero": _mutate(GOOD, 14, struct.pack("<H", 0)),
    "chunk_not_multiple_of_8": _mutate(GOOD, 22, struct.pack("<H", 44)),
    "chunk_zero": _mutate(_mutate(GOOD, 18, struct.pack("<H", 0)), 12, struct.pack("<H", 0)),
    "truncated_header": GOOD[:20],
    "header_only": GOOD[:32],
    "empty": b"",
}


def test_good_header_parses():
    assert B.parse_header(GOOD)["j"] == 9


@pytest.mark.parametrize("case", sorted(BAD))
def test_malformed_header_raises_on_the_host(case, monkeypatch):
    # any device call would go through _native.context: make it fail loudly if it is reached
    from aind_exaspim_image_compression import _native

    def no_device(*a, **k):
        raise AssertionError("a malformed stream reached the device")

    monkeypatch.setattr(_native, "context", no_device)
    with pytest.raises(ValueError):
        B.parse_header(BAD[case])
    with pytest.raises(ValueError):
        B.BoundedDctCodec(4).decode(BAD[case])


def test_codec_arguments():
    c = B.BoundedDctCodec(7)
    assert c.codec_id == "exac-dctq" and c.get_config() == {"id": "exac-dctq", "max_error": 7, "version": 1}
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            B.BoundedDctCodec(bad)


def test_store_metadata_is_read_back(tmp_path):
    """A store assembled from the restatement's chunk streams and the exac-dctq metadata reads back as the same
    container (host only: the oracle codes the chunks)."""
    rng = np.random.default_rng(3)
    shape, chunk = (20, 17, 30), (16, 8, 24)
    vol = rng.integers(900, 1100, size=shape).astype(np.uint16)
    vol[:, :8] = 1000
    streams, _, _ = ref.encode_volume(vol, chunk, 4)
    meta = chunk_store.metadata(shape, chunk, codec=B.BoundedDctCodec(4))
    assert meta["data_type"] == "uint16"
    assert meta["codecs"] == [{"name": "exac-dctq",
                               "configuration": {"version": 1, "max_error": 4, "edge_chunks": "truncated"}}]
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
    assert meta2["codecs"][0]["name"] == "exac-dctq"
    assert enc.shape == shape and enc.chunk == chunk and enc.typesize == 2
    assert [enc.chunk_bytes(i) for i in range(len(streams))] == streams
    assert np.all(enc.offsets % 16 == 0)
    steps = B.BoundedDctCodec.chunk_steps(enc)
    for s, blob in zip(steps, streams):
        assert s == (0.0 if blob[3] == 0 else B.LADDER[blob[4]])
    # the restatement's own decoder keeps its guarantee on these streams
    for s, blob in zip(ref.chunk_slices(shape, chunk), streams):
        d = ref.decode_chunk(blob)
        assert np.abs(d.astype(np.int64) - vol[s].astype(np.int64)).max() <= 4
    # a wrong configuration is refused like every other unsupported store
    meta["codecs"][0]["configuration"]["version"] = 2
    with open(os.path.join(path, "zarr.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError):
        chunk_store.read_encoded(path)
