"""The numpy restatement of the ``exac-labels`` format (tests/label_pyref.py) against itself: round
trips, every block class on both sides of its boundary, and what ``validate`` rejects (CPU)."""
import struct

import numpy as np
import pytest

import label_pyref as ref

DTYPES = (np.uint32, np.uint64)


def _ids(dtype):
    top = 2 ** (8 * np.dtype(dtype).itemsize) - 1
    return [0, 2 ** 32 - 1, top] + ([2 ** 32] if top > 2 ** 32 else [])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(16, 16, 16), (8, 8, 8), (1, 1, 1), (20, 9, 13)])
def test_round_trip(dtype, shape):
    rng = np.random.default_rng(sum(shape))
    ids = np.array(_ids(dtype) + [5, 6, 7, 1 << 20], dtype=dtype)
    smooth = ids[rng.integers(0, len(ids), shape) * (rng.random(shape) < 0.3)]        # mostly ids[0], some others
    noisy = rng.integers(0, 2 ** 31, shape).astype(dtype) * np.dtype(dtype).type(3)   # every block raw or 8 bits
    for chunk in (smooth, noisy, np.full(shape, ids[2], dtype=dtype)):
        blob = ref.encode(chunk)
        assert ref.validate(blob) == (np.dtype(dtype).itemsize, shape)
        back = ref.decode(blob)
        assert back.dtype == np.dtype(dtype) and back.shape == shape
        assert np.array_equal(back, chunk)
        assert ref.encode(back) == blob


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_class_on_both_sides_of_its_boundary(dtype):
    vol = ref.class_volume(dtype=dtype)
    for v in _ids(dtype):
        assert (vol == v).any(), f"id {v} is missing from the class volume"
    blob = ref.encode(vol)
    at, k, bits = ref.table(blob)
    ts = np.dtype(dtype).itemsize
    # a condition on the input: exactly these distinct counts occur ...
    distinct = set()
    for z in range(0, vol.shape[0], 8):
        for y in range(0, vol.shape[1], 8):
            for x in range(0, vol.shape[2], 8):
                distinct.add(len(np.unique(vol[z:z + 8, y:y + 8, x:x + 8])))
    assert {1, 2, 3, 4, 5, 16, 17, 256, 257, 512} <= distinct
    # ... so every class is in the table, the boundaries falling where the format puts them
    assert set(bits.tolist()) == {0, 1, 2, 4, 8, 8 * ts}
    for count, want in ((1, 0), (2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (256, 8)):
        assert want in bits[k == count].tolist(), (count, want)
    assert np.count_nonzero(bits == 8 * ts) >= 2 and not k[bits == 8 * ts].any()
    # at least one truncated block (the x blocks 16..18 are 3 wide) in a non-zero class
    nbx = -(-vol.shape[2] // 8)
    truncated = np.arange(len(bits)) % nbx == nbx - 1
    assert vol.shape[2] % 8 and (bits[truncated] > 0).any()
    assert np.array_equal(ref.decode(blob), vol)


def _valid(dtype=np.uint64):
    return ref.encode(ref.class_volume((16, 16, 11), dtype=dtype, counts=(1, 3, 17, 512)))


def _patched(blob, at, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, *values)
    return bytes(b)


def test_validate_accepts_what_encode_writes():
    for dtype in DTYPES:
        assert ref.validate(_valid(dtype), np.dtype(dtype).itemsize, (16, 16, 11))


def test_validate_rejects():
    blob = _valid()
    nblocks = struct.unpack_from("<I", blob, 20)[0]
    at, k, bits = ref.table(blob)
    mixed = int(np.flatnonzero(bits == 2)[0])           # a block of 3 or 4 values
    bad = {
        "magic": _patched(blob, 0, "<4s", b"EXLC"),
        "version": _patched(blob, 4, "<H", 2),
        "typesize": _patched(blob, 6, "<H", 4),
        "offset past the end": _patched(blob, ref.HEADER + 8 * (nblocks - 1), "<I", len(blob) // 8),
        "non-ascending offsets": _patched(_patched(blob, ref.HEADER + 8, "<I", int(at[2])),
                                          ref.HEADER + 16, "<I", int(at[1])),
        "k against bits": _patched(blob, ref.HEADER + 8 * mixed + 4, "<H", 5),
        "bits against k": _patched(blob, ref.HEADER + 8 * mixed + 6, "<B", 4),
        "total": _patched(blob, 24, "<I", len(blob) - 8),
        "truncated": blob[:-8],
        "truncated header": blob[:16],
        "extent": _patched(blob, 8, "<I", 17),
    }
    for name, b in bad.items():
        with pytest.raises(ValueError):
            ref.validate(b)
        with pytest.raises(ValueError):
            ref.decode(b)
    with pytest.raises(ValueError):
        ref.validate(blob, typesize=4)
    with pytest.raises(ValueError):
        ref.validate(blob, extent=(16, 16, 12))


def test_decode_rejects_an_index_outside_its_palette():
    blob = _valid()
    at, k, bits = ref.table(blob)
    b = int(np.flatnonzero((bits == 2) & (k == 3))[0])
    p = 8 * int(at[b]) + (3 * 8 + 7) // 8 * 8
    hurt = _patched(blob, p, "<B", 0xFF)                # four slots of index 3 in a palette of 3
    ref.validate(hurt)                                  # header and table are untouched
    with pytest.raises(ValueError):
        ref.decode(hurt)
