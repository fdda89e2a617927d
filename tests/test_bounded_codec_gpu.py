"""Error-bounded lossy chunk codec on the GPU: chunk streams byte-identical to the CPU
restatement (tests/bounded_pyref.py, built from the oracle's quantiser and EXAC coder), reconstructions equal to
it, the bound asserted voxel by voxel, the ladder table, per-chunk steps, the store and the metric front ends."""
import numpy as np
import pytest

import bounded_pyref as ref
from util import synth_volume

from aind_exaspim_image_compression.utils import chunk_store, img_util
from aind_exaspim_image_compression.utils import dct_quant
from aind_exaspim_image_compression.utils.bounded_codec import LADDER, BoundedDctCodec
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume, ExacCodec

pytestmark = pytest.mark.gpu

CASES = [((64, 64, 64), (64, 64, 64)), ((100, 130, 70), (64, 64, 64)), ((8, 8, 8), (64, 64, 64)),
         ((1, 1, 1), (64, 64, 64)), ((7, 8, 9), (64, 64, 64)), ((200, 64, 72), (32, 64, 48))]
DELTAS = [0, 1, 2, 4, 16, 64]
_cache = {}


def volume(shape):
    vol = synth_volume(shape, seed=sum(shape), as_u16=True)[0]
    flat = vol.reshape(-1)
    flat[:: max(1, flat.size // 9)] = 65535                 # saturating voxels
    flat[3:: max(1, flat.size // 7)] = 0
    return vol


def restated(shape, chunk):
    """(volume, restatement ladder) per case, computed once."""
    key = (shape, chunk)
    if key not in _cache:
        vol = volume(shape)
        _cache[key] = (vol, ref.volume_ladder(vol, chunk))
    return _cache[key]


def streams_of(enc):
    return [enc.chunk_bytes(i) for i in range(len(enc.sizes))]


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("shape,chunk", CASES)
def test_streams_and_reconstruction_match_the_restatement(oracle, shape, chunk, delta):
    vol, errs = restated(shape, chunk)
    want, want_rec, _ = ref.encode_volume(vol, chunk, delta, errs)
    codec = BoundedDctCodec(delta)
    enc = codec.encode_volume(vol, chunk)
    assert enc.chunk == chunk and enc.shape == shape
    got = streams_of(enc)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"chunk {k}: {len(g)} bytes, restatement {len(w)} (modes {g[3]} / {w[3]})"
    np.testing.assert_array_equal(enc.sizes, [len(w) for w in want])
    assert np.all(enc.offsets % 16 == 0)
    dec = codec.decode_volume(enc)
    np.testing.assert_array_equal(dec, want_rec)
    err = np.abs(dec.astype(np.int64) - vol.astype(np.int64))
    assert int(err.max()) <= delta
    if delta == 0:
        np.testing.assert_array_equal(dec, vol)


@pytest.mark.parametrize("shape,chunk", CASES)
def test_ladder_errors_match_the_restatement(oracle, shape, chunk):
    vol, errs = restated(shape, chunk)
    got = BoundedDctCodec(0).ladder_errors(vol, chunk)
    assert got.dtype == np.uint32 and got.shape == errs.shape
    np.testing.assert_array_equal(got, errs)


def flat_and_textured():
    rng = np.random.default_rng(11)
    shape = (64, 64, 128)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    smooth = 1000.0 + 3.0 * np.sin(zz / 19.0) + 2.0 * np.cos(yy / 23.0)
    vol = smooth + np.where(xx >= 64, rng.normal(0, 40.0, shape), 0.0)
    return np.rint(np.clip(vol, 0, 65535)).astype(np.uint16)


def test_chunks_take_their_own_steps():
    vol = flat_and_textured()
    delta = 4
    codec = BoundedDctCodec(delta)
    enc = codec.encode_volume(vol, (64, 64, 64))
    steps = BoundedDctCodec.chunk_steps(enc)
    assert len(set(steps.tolist())) == 2 and steps[0] > steps[1], steps
    dec = codec.decode_volume(enc)
    assert int(np.abs(dec.astype(np.int64) - vol).max()) <= delta
    # the best single ladder step that meets the bound everywhere, coded with the existing DCT path
    errs = codec.ladder_errors(vol, (64, 64, 64)).reshape(-1, 29)
    ok = [j for j in range(29) if np.all(errs[:, j] <= delta)]
    assert ok
    q = float(LADDER[max(ok)])
    idx = dct_quant.quantise(vol, q)
    nblk = idx.shape[0] * idx.shape[1] * idx.shape[2]
    rec = dct_quant.reconstruct(idx, vol.shape, q)
    assert int(np.abs(rec.astype(np.int64) - vol).max()) <= delta
    global_bytes = int(ExacCodec(4).chunk_sizes(idx.reshape(nblk, 8, 64), dct_quant.INDEX_CHUNK).sum())
    assert enc.nbytes < global_bytes, (enc.nbytes, global_bytes)


def test_single_chunk_encode_and_cratio(oracle):
    vol = volume((128, 64, 128))
    codec = BoundedDctCodec(2)
    enc = codec.encode_volume(vol, (64, 64, 64))
    for k, s in enumerate(ref.chunk_slices(vol.shape, (64, 64, 64))):
        blob = codec.encode(vol[s])
        assert blob == enc.chunk_bytes(k)
        np.testing.assert_array_equal(codec.decode(blob).reshape(vol[s].shape), ref.decode_chunk(blob))
    # a ragged chunk alone: nominal shape = extent rounded up to multiples of 8
    part = np.ascontiguousarray(vol[:13, :20, :7])
    blob = codec.encode(part)
    assert blob[18:24] == np.array([16, 24, 8], dtype="<u2").tobytes()
    assert blob == ref.encode_chunk(part, (16, 24, 8), 2)[0]
    assert int(np.abs(codec.decode(blob).reshape(part.shape).astype(np.int64) - part).max()) <= 2
    assert img_util.compute_cratio(vol, codec) == round(vol.nbytes / int(enc.sizes.sum()), 2)
    np.testing.assert_array_equal(codec.chunk_sizes(vol, (64, 64, 64)), enc.sizes)


def test_store_round_trip(tmp_path):
    vol = volume((100, 130, 70))
    codec = BoundedDctCodec(4)
    path = str(tmp_path / "bounded.zarr")
    cr = chunk_store.write_zarr(vol, path, codec=codec)
    enc = codec.encode_volume(vol, (64, 64, 64))
    assert cr == pytest.approx(vol.nbytes / enc.nbytes)
    back = chunk_store.read_zarr(path)
    assert back.shape == (1, 1) + vol.shape
    np.testing.assert_array_equal(back[0, 0], codec.decode_volume(enc))
    assert int(np.abs(back[0, 0].astype(np.int64) - vol).max()) <= 4
    np.testing.assert_array_equal(chunk_store.read_chunk(path, 1, 2, 1), back[0, 0, 64:, 128:, 64:])
    # the lossless default store is untouched by the new codec
    path2 = str(tmp_path / "exac.zarr")
    chunk_store.write_zarr(vol, path2)
    np.testing.assert_array_equal(chunk_store.read_zarr(path2)[0, 0], vol)


def test_compress_and_decompress_is_encode_plus_decode():
    vol = volume((100, 130, 70))
    codec = BoundedDctCodec(16)
    dec, cr = img_util.compress_and_decompress(vol[np.newaxis, np.newaxis], codec)
    enc = codec.encode_volume(vol, (64, 64, 64))
    assert dec.shape == (1, 1) + vol.shape
    np.testing.assert_array_equal(dec[0, 0], codec.decode_volume(enc))
    assert cr == round(vol.nbytes / enc.nbytes, 2) == img_util.compute_cratio(vol, codec)
    dec3, cr3 = img_util.compress_and_decompress(vol, ExacCodec(2))
    np.testing.assert_array_equal(dec3, vol)
    assert cr3 == img_util.compute_cratio(vol, ExacCodec(2))


def test_malformed_containers_are_refused_on_the_device():
    vol = flat_and_textured()
    codec = BoundedDctCodec(4)
    enc = codec.encode_volume(vol, (64, 64, 64))
    assert enc.chunk_bytes(0)[3] == 1                   # the flat chunk is stored lossy

    def with_data(data):
        return EncodedVolume(data, enc.offsets.copy(), enc.sizes.copy(), enc.shape, enc.chunk, 2)

    swapped = enc.data.copy()                  # the lossy chunk claims a lossless payload
    o = int(enc.offsets[0])
    swapped[o + 3], swapped[o + 4], swapped[o + 8:o + 12] = 0, 0xFF, 0
    bad_q = enc.data.copy()
    bad_q[o + 8:o + 12] = np.frombuffer(LADDER[0].tobytes(), np.uint8)
    bad_e = enc.data.copy()
    bad_e[o + 12] = 63
    payload = enc.data.copy()                  # an EXAC payload of uint16 elements behind a lossy header
    payload[o + 32 + 3] = 2
    for data in (swapped, bad_q, bad_e, payload):
        with pytest.raises(ValueError):
            codec.decode_volume(with_data(data))
    short = EncodedVolume(enc.data[:int(enc.offsets[1]) + 32], enc.offsets.copy(), enc.sizes, enc.shape, enc.chunk, 2)
    with pytest.raises(ValueError):
        codec.decode_volume(short)
    np.testing.assert_array_equal(codec.decode_volume(enc), codec.decode_volume(with_data(enc.data.copy())))


def test_realistic_chunk_count(oracle):
    vol = synth_volume((256, 256, 256), seed=256, as_u16=True)[0]
    chunk = (64, 64, 64)
    errs = ref.volume_ladder(vol, chunk)
    codec = BoundedDctCodec(4)
    np.testing.assert_array_equal(codec.ladder_errors(vol, chunk), errs)
    want, want_rec, steps = ref.encode_volume(vol, chunk, 4, errs)
    enc = codec.encode_volume(vol, chunk)
    assert streams_of(enc) == want
    np.testing.assert_array_equal(codec.decode_volume(enc), want_rec)
    assert int(np.abs(want_rec.astype(np.int64) - vol).max()) <= 4
