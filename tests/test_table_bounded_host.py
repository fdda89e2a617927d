"""Block-bounded codec with a bound table, host side: ``noise.bound_table`` against the formula, the
restatement with a constant table against the table-less one, the codec's arguments and configuration, and the chunk
store's ``"bound"`` metadata.  No GPU."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import block_bounded_pyref as base
import table_bounded_pyref as ref

from aind_exaspim_image_compression.utils import block_bounded_codec as B
from aind_exaspim_image_compression.utils import chunk_store
from aind_exaspim_image_compression.utils import noise as N

PARAMS = [ref.NOISE, {"gain": 0.37, "read_noise": 1.9, "offset": 512.5}]


def _direct(p, k, c, cap=65535):
    return min(cap, math.floor(k * math.sqrt(p["gain"] * max(c - p["offset"], 0.0) + p["read_noise"] ** 2)))


@pytest.mark.parametrize("p", PARAMS, ids=["g2-r3-o100", "g0.37-r1.9-o512.5"])
@pytest.mark.parametrize("k", [0.5, 2.0, 7.25])
def test_bound_table_is_the_formula(p, k):
    t = N.bound_table(p, k)
    assert t.dtype == np.uint16 and t.shape == (65536,)
    off = int(p["offset"])
    for c in (0, off - 1, off, off + 1, 1000, 65535):
        assert int(t[c]) == _direct(p, k, c), c
    assert np.all(np.diff(t.astype(np.int64)) >= 0)
    assert int(t[0]) == math.floor(k * p["read_noise"])
    np.testing.assert_array_equal(t, ref.formula_table(p, k))
    # an anscombe transform cfg is accepted like everywhere else
    np.testing.assert_array_equal(N.bound_table({"kind": "anscombe", "params": p}, k), t)


def test_bound_table_cap_and_zero():
    t = N.bound_table(ref.NOISE, 2.0)
    assert t.max() > 300
    capped = N.bound_table(ref.NOISE, 2.0, cap=300)
    np.testing.assert_array_equal(capped, np.minimum(t, 300))
    assert N.bound_table(ref.NOISE, 1e6).max() == 65535                # floor() beyond uint16 is capped, not wrapped
    assert not N.bound_table(ref.NOISE, 0.0).any()
    assert not N.bound_table(ref.NOISE, 2.0, cap=0).any()


@pytest.mark.parametrize("noise,k", [({"gain": 2.0, "read_noise": 3.0}, 0.3),
                                     (ref.NOISE, -0.5),
                                     (ref.NOISE, float("nan")),
                                     (ref.NOISE, float("inf")),
                                     ({"gain": 0.0, "read_noise": 3.0, "offset": 100.0}, 0.3),
                                     ({"gain": float("nan"), "read_noise": 3.0, "offset": 100.0}, 0.3),
                                     ("auto", 0.3)],
                         ids=["missing-key", "negative-k", "nan-k", "inf-k", "zero-gain", "nan-gain", "no-dict"])
def test_bound_table_refuses(noise, k):
    with pytest.raises(ValueError):
        N.bound_table(noise, k)
    with pytest.raises(ValueError):
        B.BlockBoundedCodec.from_noise(noise, k)


def test_bound_table_cap_range():
    for cap in (-1, 65536):
        with pytest.raises(ValueError):
            N.bound_table(ref.NOISE, 1.0, cap=cap)


@pytest.fixture(scope="module")
def main_volume():
    vol = ref.pg_volume(ref.MAIN[0])
    vol.setflags(write=False)
    return vol


def test_the_volume_is_what_the_cases_need(main_volume):
    vol = main_volume
    assert vol.dtype == np.uint16 and vol.shape == ref.MAIN[0]
    assert vol.max() == 65535 and vol.min() == 0
    body = np.delete(vol.reshape(-1), np.flatnonzero((vol.reshape(-1) == 0) | (vol.reshape(-1) == 65535)))
    assert 10000 < body.max() < 40000 and np.median(body) < 300
    dark = vol[0:8, 8:16, 0:8]
    assert int((dark > 200).sum()) == 1 and dark[3, 4, 5] == 30000


@pytest.mark.parametrize("delta", [4, 0])
def test_constant_table_is_the_constant_bound(oracle, main_volume, delta):
    """T == delta under max_error = 65535 gives exactly the table-less restatement at max_error = delta."""
    shape, chunk = ref.MAIN
    table = np.full(65536, delta, np.uint16)
    want = base.encode_volume(main_volume, chunk, delta)
    got = ref.encode_volume(main_volume, chunk, 65535, table=table)
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    for a, b in zip(got[2], want[2]):
        assert (a is None and b is None) or np.array_equal(a, b)
    for a, b in zip(ref.volume_steps(main_volume, chunk, 65535, table=table),
                    base.volume_steps(main_volume, chunk, delta)):
        np.testing.assert_array_equal(a, b)
    if delta == 0:
        np.testing.assert_array_equal(got[1], main_volume)


def test_restatement_keeps_the_table_bound(oracle, main_volume):
    shape, chunk = ref.MAIN
    rng = np.random.default_rng(5)
    mask = (rng.random(shape) < 0.1).astype(np.uint8)
    table = N.bound_table(ref.NOISE, 2.0)
    b = ref.bounds(main_volume, 8, 1, mask, table)
    np.testing.assert_array_equal(b, np.minimum(table[main_volume], np.where(mask != 0, 1, 8)))
    streams, rec, _ = ref.encode_volume(main_volume, chunk, 8, 1, mask, table)
    assert np.all(np.abs(rec.astype(np.int64) - main_volume) <= b)
    for s, blob in zip(ref.chunk_slices(shape, chunk), streams):
        np.testing.assert_array_equal(ref.decode_chunk(blob), rec[s])


def test_the_table_binds_differently_across_intensity(oracle, main_volume):
    """With bound_table(k = 2) and max_error = 65535 the restatement's step varies over the inside blocks, and the
    dark block with one bright voxel takes a finer step than its neighbours; without the table every inside block
    takes the coarsest step.  What test_table_bounded_gpu.py's test_the_step_follows_the_intensity relies on."""
    shape, chunk = ref.MAIN
    st = np.stack(ref.volume_steps(main_volume, chunk, 65535, table=N.bound_table(ref.NOISE, 2.0)))
    assert len(set(st[st >= 0].tolist())) >= 4 and not (st == -1).any()
    assert st[0, 0, 1, 0] < st[0, 0, 0, 0] and st[0, 0, 1, 0] < st[0, 0, 1, 1]
    loose = np.stack(base.volume_steps(main_volume, chunk, 65535))
    assert set(loose[loose != -2].tolist()) == {base.STEPS - 1}


def test_codec_arguments():
    c = B.BlockBoundedCodec()
    assert (c.max_error, c.fg_max_error, c.bound_table, c.bound) == (65535, 65535, None, None)
    assert "bound" not in c.get_config()
    table = np.arange(65536, dtype=np.uint16)
    c = B.BlockBoundedCodec(9, 2, bound_table=table)
    assert (c.max_error, c.fg_max_error) == (9, 2)
    np.testing.assert_array_equal(c.bound_table, table)
    table[7] = 0                                        # the codec keeps its own copy
    assert c.bound_table[7] == 7
    sha = hashlib.sha256(np.arange(65536, dtype="<u2").tobytes()).hexdigest()
    assert c.get_config() == {"id": "exac-dctq-block", "max_error": 9, "fg_max_error": 2, "version": 1,
                              "bound": {"kind": "table", "sha256": sha}}
    for bad in (np.zeros(65536, np.int16), np.zeros(65535, np.uint16), np.zeros((65536, 1), np.uint16),
                np.zeros(65536, np.float32), list(range(65536)), np.zeros((2, 32768), np.uint16)):
        with pytest.raises(ValueError):
            B.BlockBoundedCodec(9, 2, bound_table=bad)
    with pytest.raises(ValueError):
        B.BlockBoundedCodec(4, 5, bound_table=np.zeros(65536, np.uint16))


def test_from_noise():
    p = {"gain": 1.5, "read_noise": 2.25, "offset": 99.0}
    c = B.BlockBoundedCodec.from_noise(p, 0.5)
    assert (c.max_error, c.fg_max_error) == (65535, 65535)
    np.testing.assert_array_equal(c.bound_table, N.bound_table(p, 0.5))
    assert c.get_config()["bound"] == {"kind": "poisson-gaussian", "gain": 1.5, "read_noise": 2.25, "offset": 99.0,
                                       "k": 0.5}
    c = B.BlockBoundedCodec.from_noise({"kind": "anscombe", "params": p}, 2, max_error=40, fg_max_error=3)
    assert (c.max_error, c.fg_max_error) == (40, 3)
    np.testing.assert_array_equal(c.bound_table, N.bound_table(p, 2.0))
    assert c.get_config()["bound"]["k"] == 2.0 and c.get_config()["bound"]["gain"] == 1.5
    json.dumps(c.get_config())                          # plain floats and strings


def test_encode_device_wants_the_table_with_the_codec(monkeypatch):
    """A codec with a table refuses a device encode without one (and the other way round) before any device call."""
    from aind_exaspim_image_compression import _native

    def no_device(*a, **k):
        raise AssertionError("reached the device")

    monkeypatch.setattr(_native, "block_bounded_volume_bound", no_device)
    with pytest.raises(ValueError):
        B.BlockBoundedCodec(bound_table=np.zeros(65536, np.uint16)).encode_device(None, 1, (8, 8, 8), (8, 8, 8))
    with pytest.raises(ValueError):
        B.BlockBoundedCodec(4).encode_device(None, 1, (8, 8, 8), (8, 8, 8), d_table=2)


def _write_store(path, meta, streams, g):
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


def test_store_metadata_carries_the_bound(oracle, tmp_path):
    """A one-chunk store written by hand from the restatement's stream: ``metadata`` writes ``"bound"`` next to the
    two errors, and ``read_encoded`` / ``_codec_of`` read the store with the key, without it, and with a key they
    have never heard of."""
    shape = chunk = (8, 16, 24)
    vol = ref.pg_volume((16, 16, 24))[:8]
    codec = B.BlockBoundedCodec.from_noise(ref.NOISE, 0.5, max_error=50, fg_max_error=2)
    streams, rec, _ = ref.encode_volume(vol, chunk, 50, 2, None, codec.bound_table)
    assert len(streams) == 1
    meta = chunk_store.metadata(shape, chunk, codec=codec)
    cfg = meta["codecs"][0]["configuration"]
    assert meta["codecs"][0]["name"] == "exac-dctq-block"
    assert cfg == {"version": 1, "max_error": 50, "fg_max_error": 2, "edge_chunks": "truncated",
                   "bound": {"kind": "poisson-gaussian", "gain": 2.0, "read_noise": 3.0, "offset": 100.0, "k": 0.5}}
    bare = B.BlockBoundedCodec(50, 2, bound_table=codec.bound_table)
    assert chunk_store.metadata(shape, chunk, codec=bare)["codecs"][0]["configuration"]["bound"] == \
        {"kind": "table", "sha256": hashlib.sha256(codec.bound_table.astype("<u2").tobytes()).hexdigest()}
    assert "bound" not in chunk_store.metadata(shape, chunk, codec=B.BlockBoundedCodec(50, 2))["codecs"][0][
        "configuration"]
    without = json.loads(json.dumps(meta))
    del without["codecs"][0]["configuration"]["bound"]
    unknown = json.loads(json.dumps(meta))
    unknown["codecs"][0]["configuration"]["bound"] = {"kind": "something-newer", "x": [1, 2]}
    for i, m in enumerate((meta, without, unknown)):
        path = str(tmp_path / f"store{i}")
        _write_store(path, m, streams, (1, 1, 1))
        enc, meta2 = chunk_store.read_encoded(path)
        assert enc.shape == shape and enc.chunk == chunk and enc.typesize == 2
        assert enc.chunk_bytes(0) == streams[0]
        picked = chunk_store._codec_of(meta2)
        assert isinstance(picked, B.BlockBoundedCodec) and (picked.max_error, picked.fg_max_error) == (50, 2)
        assert picked.bound_table is None               # the decoder needs no table
        np.testing.assert_array_equal(ref.decode_chunk(enc.chunk_bytes(0)), rec)
    # write_encoded writes the same entry
    enc, _ = chunk_store.read_encoded(str(tmp_path / "store0"))
    chunk_store.write_encoded(enc, str(tmp_path / "again"), codec=codec)
    with open(os.path.join(str(tmp_path / "again"), "zarr.json")) as f:
        assert json.load(f)["codecs"] == meta["codecs"]
