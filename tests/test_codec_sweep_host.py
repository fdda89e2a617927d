"""CPU: the inputs of the chunk-coder sweep (tests/codec_sweep_cases.py).  The oracle's v2 stream of every chunk
of every case decodes to the input in both decoders -- tests/exac2_pyref.py, written from the format text, and the C
decoder -- and a census over those streams' headers shows that the table reaches what the GPU sweep
(tests/test_codec_sweep_gpu.py) is there to reach: every symbol and context of both element kinds, wide
frequencies, single-symbol contexts inside coded streams, streams without words, and each of the three model
kernels.  These are conditions on the inputs, not on the GPU code."""
import numpy as np
import pytest

import exac2_pyref
from codec_sweep_cases import CASES, PAIRS, BY_NAME, census, chunk_index_map, form_of, oracle_streams, volume
from oracle import codec_oracle as co

IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_streams_decode_in_both_decoders(case):
    name, dtype, shape, chunk, kind = case
    vol = volume(case)
    streams = oracle_streams(case)
    chunks = list(co.chunks(vol, chunk))
    assert len(streams) == len(chunks)
    for i, (b, c) in enumerate(zip(streams, chunks)):
        got, shp = exac2_pyref.decode(b)
        assert shp == co.shape3(c.shape), (name, i)
        np.testing.assert_array_equal(got, c.reshape(-1), err_msg=f"{name}: chunk {i}, Python decoder")
        back, used = co.decode(b, c.size, c.dtype.itemsize)
        assert used == len(b)
        np.testing.assert_array_equal(back, c.reshape(-1), err_msg=f"{name}: chunk {i}, C decoder")


def test_routing_pairs_hold_the_same_chunks():
    """The generic-routed volume of a pair holds the chunks of the other one, and the oracle -- which only ever
    sees a chunk -- codes them to the same bytes."""
    for a, b in PAIRS:
        ca, cb = BY_NAME[a], BY_NAME[b]
        ts = np.dtype(ca[1]).itemsize
        assert form_of(ts, ca[2], ca[3]) in ("strips", "rows32") and form_of(ts, cb[2], cb[3]) == "generic"
        sa, sb = oracle_streams(ca), oracle_streams(cb)
        pairs = chunk_index_map(ca, cb)
        assert len(pairs) == len(sa)
        for i, j in pairs:
            assert sa[i] == sb[j], (a, i, j)


def test_coverage_census():
    """What the table reaches, read from the `present` / `wide` bitmaps and `nwords` of the oracle's own headers."""
    seen = {2: [0] * 16, 4: [0] * 16}                 # element size -> per context, the union of `present`
    wide_bits = single_in_coded = wordless = 0
    forms = {"strips": 0, "rows32": 0, "generic": 0}
    for case in CASES:
        ts = np.dtype(case[1]).itemsize
        forms[form_of(ts, case[2], case[3])] += 1
        for b in oracle_streams(case):
            h = census(b)
            for q in range(16):
                seen[ts][q] |= h["present"][q]
                wide_bits += bin(h["wide"][q]).count("1")
                if h["nwords"] > 0 and bin(h["present"][q]).count("1") == 1:
                    single_in_coded += 1
            wordless += h["nwords"] == 0
    union = {ts: 0 for ts in seen}
    for ts in seen:
        for q in range(16):
            union[ts] |= seen[ts][q]
    missing16 = [s for s in range(46) if not union[2] >> s & 1]
    missing32 = [s for s in range(62) if not union[4] >> s & 1]
    print("census: uint16 symbols missing", missing16, "int32 symbols missing", missing32,
          "empty contexts", {ts: [q for q in range(16) if not seen[ts][q]] for ts in seen},
          "wide", wide_bits, "single-symbol contexts in coded streams", single_in_coded, "wordless", wordless, forms)
    assert not missing16, f"uint16 symbols never coded: {missing16}"
    assert union[2] >> 46 == 0
    assert not missing32, f"int32 symbols never coded: {missing32}"
    assert union[4] >> 62 == 0
    for ts in seen:
        assert all(seen[ts][q] for q in range(16)), f"typesize {ts}: an empty context"
    assert wide_bits >= 1
    assert single_in_coded >= 1
    assert wordless >= 1
    assert all(v >= 4 for v in forms.values()), forms
