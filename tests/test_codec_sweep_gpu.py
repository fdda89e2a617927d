"""The GPU chunk coders (csrc/rans2_kernels.hip: EXAC v2; csrc/rans_kernels.hip: EXAC v1 and the offset scan both
share) over the table of tests/codec_sweep_cases.py: every model kernel of the v2 encoder (strips, rows32, generic)
at the chunk extents where it branches, every symbol class and context, tap distances at the format's limit, more
than 1024 chunks, and the 120 fuzz chunks the C encoder gets on the CPU.  tests/test_codec_sweep_host.py shows on the
CPU that the table reaches all of that and that the oracle's streams are right.  Every comparison is an equality
with the oracle (oracle/exac_codec.c) or with the input."""
import numpy as np
import pytest

from codec_sweep_cases import BY_NAME, CASES, PAIRS, chunk_index_map, form_of, fuzz_chunks, oracle_streams, volume
from test_codec_buffers_gpu import layout_container
from test_codec_gpu import check_against_oracle

from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume, ExacCodec
from oracle import codec_oracle as co

pytestmark = pytest.mark.gpu
VERSIONS = pytest.mark.parametrize("version", [2, 1])


@VERSIONS
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_volume_sweep(case, version):
    name, dtype, shape, chunk, kind = case
    vol = volume(case)
    ts = vol.dtype.itemsize
    codec = ExacCodec(ts, version=version)
    enc = codec.encode_volume(vol, chunk)
    check_against_oracle(enc, vol, chunk, version)              # streams, exact sizes, zero pads
    want = oracle_streams(case, version)
    data, offsets, sizes = layout_container(want)
    np.testing.assert_array_equal(enc.offsets, offsets)         # the running 16-byte-aligned sums
    np.testing.assert_array_equal(enc.sizes, sizes)
    np.testing.assert_array_equal(enc.data, data)
    np.testing.assert_array_equal(codec.chunk_sizes(vol, chunk), sizes)
    np.testing.assert_array_equal(codec.decode_volume(enc).reshape(shape), vol)
    # the oracle's own streams, laid out on the host, through the GPU decoder
    theirs = EncodedVolume(data, offsets, sizes, enc.shape, enc.chunk, ts)
    np.testing.assert_array_equal(codec.decode_volume(theirs).reshape(shape), vol)


@pytest.mark.parametrize("pair", PAIRS, ids=[p[0] for p in PAIRS])
def test_routing_pairs_give_identical_chunk_bytes(pair):
    """The three model kernels share one contract: a chunk's bytes do not depend on which of them modelled it.
    The second volume of a pair holds the chunks of the first and more columns, so that nx % 64 != 0 (uint16) or
    nx % cx != 0 (int32) sends it to the generic kernel."""
    a, b = BY_NAME[pair[0]], BY_NAME[pair[1]]
    ts = np.dtype(a[1]).itemsize
    assert form_of(ts, a[2], a[3]) != "generic" and form_of(ts, b[2], b[3]) == "generic"
    codec = ExacCodec(ts)
    ea, eb = codec.encode_volume(volume(a), a[3]), codec.encode_volume(volume(b), b[3])
    for i, j in chunk_index_map(a, b):
        assert ea.chunk_bytes(i) == eb.chunk_bytes(j), f"chunk {i} of {a[0]} / chunk {j} of {b[0]}"


@VERSIONS
def test_fuzz_chunks_against_the_oracle(version):
    for it, shape, a in fuzz_chunks():
        codec = ExacCodec(a.dtype.itemsize, version=version)
        want = co.encode(a, version=version)
        assert codec.encode(a) == want, f"iteration {it}, shape {shape}, {a.dtype}"
        np.testing.assert_array_equal(codec.decode(want), a.reshape(-1), err_msg=f"iteration {it}, shape {shape}")
