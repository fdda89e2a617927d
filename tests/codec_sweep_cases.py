"""Inputs of the chunk-coder sweep (tests/test_codec_sweep_host.py on the CPU, tests/test_codec_sweep_gpu.py on the
GPU): a table of small volumes that between them reach every model kernel of the EXAC v2 encoder
(csrc/rans2_kernels.hip: strips, rows32, generic) at the geometries where those kernels branch, every symbol and
context of the format, the chunk-count branches of the offset scan, and the tap distances around
the format's limit of 8000 elements.  Helper, not a test.

A case is ``(name, dtype, volume shape, chunk, data kind)``; ``volume(case)`` builds its array (cached, read-only),
``oracle_streams(case, version)`` the oracle's stream of every chunk (cached)."""
import zlib

import numpy as np

from oracle import codec_oracle as co

U16, I32 = np.uint16, np.int32


# ---- the 120 fuzz chunks of test_oracle_codec.py ----------------------------------------------------------------------
def fuzz_chunks():
    """120 random small chunks -- shapes with rows narrower and wider than a wave, planes smaller than a row, both
    element kinds, flat / noisy / spiky / extreme data.  Yields (iteration, shape, array); seed 20261006."""
    rng = np.random.default_rng(20261006)
    for it in range(120):
        shape = tuple(int(v) for v in rng.integers(1, [7, 12, 90]))
        kind = int(rng.integers(0, 5))
        if rng.random() < 0.5:
            base = rng.normal(rng.choice([0, 37, 3000, 60000]), rng.choice([0.0, 1.0, 4.0, 40.0, 900.0]), shape)
            a = np.clip(base, 0, 65535).round().astype(np.uint16)
            if kind == 0:
                a.reshape(-1)[:: int(rng.integers(2, 9))] = rng.integers(0, 65536)
        else:
            a = rng.laplace(0, rng.choice([0.3, 2.0, 50.0, 1e5]), shape).round().astype(np.int64)
            a = np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
            if kind == 1:
                a.reshape(-1)[0] = -2 ** 31
        yield it, shape, a


# ---- stream header -----------------------------------------------------------------------------------------------------
def census(stream):
    """v2 stream header (layout: oracle/exac_codec.c) -> {"nwords", "present": 16 bitmaps, "wide": 16 bitmaps}."""
    b = bytes(stream)
    assert b[:3] == b"EX\x02" and len(b) >= 276
    return {"nwords": int.from_bytes(b[16:20], "little"),
            "present": [int.from_bytes(b[20 + 8 * c:28 + 8 * c], "little") for c in range(16)],
            "wide": [int.from_bytes(b[148 + 8 * c:156 + 8 * c], "little") for c in range(16)]}


# ---- which model kernel codes a volume ------------------------------------------------------------------------------------
def form_of(ts, shape, chunk):
    """The model kernel launch_rans2_encode (csrc/rans2_kernels.hip) picks for a volume: "strips", "rows32" or
    "generic".  This restates the three conditions of that function and the two mirror each other: change them
    together.  (The chunk is clamped to the volume first, as make_codec_geom does.)"""
    nz, ny, nx = shape
    cz, cy, cx = (min(int(c), int(s)) for c, s in zip(chunk, shape))
    if ts == 2 and cx == 64 and nx % 64 == 0 and cy <= 64:        # STRIP * MODEL_WAVES = 64
        return "strips"
    if ts == 4 and cx % 64 == 0 and nx % cx == 0:
        return "rows32"
    return "generic"


# ---- data kinds ------------------------------------------------------------------------------------------------------------
def _unzigzag(u):
    return (u >> 1) ^ -(u & 1)


def value_of_symbol(s, e=0):
    """A residual (as a signed integer) that the v2 alphabet codes as symbol s with raw value e."""
    u = s if s < 32 else 32 + (((1 << (s - 32)) - 1) << 2) + e
    return _unzigzag(u)


def _denoised(rng, shape, dtype):
    if dtype == U16:        # the family of tests/test_codec_gpu.py: Gaussian, sparse spikes, a few 65535s
        a = np.clip(rng.normal(37, 2.0, shape), 0, 65535)
        zz = np.arange(shape[0])[:, None, None]
        a = a + 900.0 * np.exp(-((zz - shape[0] / 2.0) ** 2) / 18.0) * (rng.random(shape) < 0.3)
        a = np.rint(a).astype(U16)
        a.reshape(-1)[:: max(1, a.size // 11)] = 65535
        return a
    a = rng.laplace(0, 2.0, shape).round().astype(np.int64)       # quantisation-index like
    flat = a.reshape(-1)
    flat[5::97] = rng.integers(-3000, 3000, flat[5::97].size)
    return a.astype(I32)


def _octaves16(rng, shape, dtype):
    """2^k - 1 + {0, 1, 2} on the even rows, zero on the odd ones: the residuals span every octave."""
    k = rng.integers(0, 17, shape)
    a = np.minimum((1 << k) - 1 + rng.integers(0, 3, shape), 65535)
    rows = np.arange(int(np.prod(shape[:2]))).reshape(shape[:2])
    a[rows % 2 == 1] = 0
    return a.astype(U16)


def _wrap16(rng, shape, dtype):
    """0 / 65535 / 32768 in turn: |v - P| >= 32768, the residual wraps in int16."""
    return np.resize(np.array([0, 65535, 32768], dtype=U16), int(np.prod(shape))).reshape(shape)


def _octaves32(rng, shape, dtype):
    """+- 2^U(0, 31), with -2^31 and 2^31 - 1."""
    a = np.floor(2.0 ** rng.uniform(0, 31, shape)).astype(np.int64) * rng.choice([-1, 1], shape)
    flat = a.reshape(-1)
    flat[0], flat[-1] = -2 ** 31, 2 ** 31 - 1
    flat[flat.size // 2] = -2 ** 31
    return np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(I32)


def _silent(rng, shape, dtype):
    return np.full(shape, 0 if dtype == U16 else -3, dtype=dtype)


def _silent37(rng, shape, dtype):
    return np.full(shape, 37, dtype=dtype)


def _one_nonzero(rng, shape, dtype):
    a = np.zeros(shape, dtype=dtype)
    a.reshape(-1)[(2 * a.size) // 3] = 9
    return a


def _tie3(rng, shape, dtype):
    """Three symbols, equally frequent in one context: each gets floor(4096 / 3) = 1365 and the deficit of 1 goes
    to the lowest of them.  Every residual has magnitude 127, so whatever has a tap is in context 15.
    uint16 (chunks (1, 4, 64)): row 0 of a chunk is 1000, each later row is the row above plus a residual from
    {200, 300, 600}, 64 of each over rows 1..3.  int32 ((4, 4, 64)): the 960 elements behind the first row."""
    r = np.array([200, 300, 600])
    if dtype == I32:
        assert (int(np.prod(shape)) - shape[2]) % 3 == 0
        return np.resize(r, int(np.prod(shape))).reshape(shape).astype(I32)
    a = np.zeros(shape, dtype=np.int64)
    x = np.arange(shape[2])
    for y in range(shape[1]):
        a[:, y, :] = 1000 if y % 4 == 0 else a[:, y - 1, :] + r[(x + y) % 3]
    return a.astype(U16)


def _dominated(rng, shape, dtype):
    """One value next to one occurrence of every other symbol of the element kind, all in context 0 (a 1-D chunk
    has no taps): the rare symbols are forced up to F = 1 and the excess comes off the dominant one."""
    a = np.zeros(shape, dtype=np.int64)
    flat = a.reshape(-1)
    syms = np.arange(1, 46 if dtype == U16 else 62)
    assert flat.size > 4096 + syms.size
    at = 7 + 101 * np.arange(syms.size)
    flat[at] = [value_of_symbol(int(s), int(s) % 3) for s in syms]
    return (a & 0xFFFF).astype(U16) if dtype == U16 else a.astype(I32)


def _bytes256(rng, shape, dtype):
    """EXAC v1: all 256 values in both byte planes, one of them dominating (255 symbols forced up to F = 1)."""
    a = np.full(shape, 0x2525, dtype=np.int64)
    flat = a.reshape(-1)
    assert flat.size >= 16384
    flat[3 + 61 * np.arange(256)] = 257 * np.arange(256)
    return a.astype(U16)


_KINDS = {"denoised": _denoised, "octaves16": _octaves16, "wrap16": _wrap16, "octaves32": _octaves32,
          "silent": _silent, "silent37": _silent37, "one_nonzero": _one_nonzero, "tie3": _tie3,
          "dominated": _dominated, "bytes256": _bytes256}

# ---- the table -------------------------------------------------------------------------------------------------------------
CASES = []
PAIRS = []          # (case routed to strips / rows32, case with the same chunks routed to the generic kernel)
_EMBED = {}         # name of a generic-routed case -> name of the case whose volume it extends along x


def _add(name, dtype, shape, chunk, kind):
    CASES.append((name, dtype, shape, chunk, kind))


def _geom(name, shape, chunk, kinds16=("denoised",), kinds32=()):
    for k in kinds16:
        _add(f"{name}-u16-{k}", U16, shape, chunk, k)
    for k in kinds32:
        _add(f"{name}-i32-{k}", I32, shape, chunk, k)


# strips form (uint16, cx = 64, nx % 64 = 0, cy <= 64): cy around the strip of 16 rows, cz around the block of 16 planes
_geom("strips-cy1-cz4", (6, 3, 128), (4, 1, 64), ("denoised", "one_nonzero"))
_geom("strips-cy15-cz17", (18, 30, 128), (17, 15, 64), ("denoised", "wrap16"))
_geom("strips-cy16-cz15", (16, 32, 64), (15, 16, 64), ("denoised", "silent37"))
_geom("strips-cy17-cz33", (34, 34, 64), (33, 17, 64), ("denoised", "octaves16"))
_geom("strips-cy48-cz1", (3, 50, 128), (1, 48, 64), ("denoised", "octaves16"))
_geom("strips-cy63-cz17", (17, 64, 64), (17, 63, 64), ("denoised", "silent"))
_geom("strips-ragged", (37, 50, 128), (17, 33, 64), ("denoised",))
_geom("strips-tie", (2, 8, 128), (1, 4, 64), ("tie3",))
# rows32 form (int32, cx % 64 = 0, nx % cx = 0); the same geometries with uint16 go to the generic kernel
_geom("rows-3-5-128", (7, 12, 256), (3, 5, 128), ("denoised",), ("denoised", "octaves32"))       # rpx = 2, ragged
_geom("rows-4-32-320", (5, 40, 320), (4, 32, 320), ("denoised",), ("denoised", "octaves32"))    # ex <= 8000 < plane
_geom("rows-5-1-64", (11, 3, 128), (5, 1, 64), ("octaves16",), ("denoised", "one_nonzero"))
_geom("rows-513", (28, 20, 64), (27, 19, 64), ("denoised",), ("denoised", "octaves32"))         # 513 / 27 / 19 / 1 rows
_geom("rows-515", (5, 103, 64), (5, 103, 64), ("denoised",), ("denoised", "silent"))            # 515 rows, plane 6592
_geom("rows-tie", (4, 4, 64), (4, 4, 64), (), ("tie3",))
_geom("flat-8192", (1, 1, 8192), (1, 1, 8192), ("dominated",), ("dominated",))
# the tap limit and narrow rows / planes: whole-volume chunks
for _s in ((2, 3, 8000), (2, 3, 8001), (3, 125, 64), (3, 126, 64)):
    _geom("limit-%d-%d-%d" % _s, _s, _s, ("denoised", "wrap16"), ("denoised", "octaves32"))
for _s in ((3, 127, 63), (4, 7, 9), (3, 64, 1), (70, 1, 1), (2, 2, 65)):
    _geom("limit-%d-%d-%d" % _s, _s, _s, ("denoised", "octaves16"), ("octaves32",))
_geom("limit-planes", (5, 130, 200), (4, 125, 64), ("denoised",), ("denoised",))       # planes of 8000, 1000, 320, 40
_geom("limit-silent", (4, 7, 9), (4, 7, 9), ("silent", "one_nonzero"), ("silent",))
# many chunks: the offset scan with 3 and 2 chunks per thread and empty ranges in the last threads
_geom("many-2431", (13, 11, 17), (1, 1, 1), ("octaves16",), ())
_geom("many-1025", (2, 2, 2050), (2, 2, 2), ("denoised",), ("denoised",))
# EXAC v1's normalisation loop
_geom("v1-bytes", (4, 64, 64), (4, 64, 64), ("bytes256",), ())
# the chunks of a strips case and of a rows32 case inside a volume that routes to the generic kernel
for _src, _shape in (("strips-cy17-cz33-u16-octaves16", (34, 34, 65)), ("strips-cy15-cz17-u16-denoised", (18, 30, 130)),
                     ("rows-3-5-128-i32-octaves32", (7, 12, 257)), ("rows-513-i32-denoised", (28, 20, 65))):
    _c = next(c for c in CASES if c[0] == _src)
    _name = "generic-of-" + _src
    _add(_name, _c[1], _shape, _c[3], "embed")
    _EMBED[_name] = _src
    PAIRS.append((_src, _name))

BY_NAME = {c[0]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_cache = {}


def volume(case):
    """The case's array (cached; read-only so that no test changes what another one compares with)."""
    name, dtype, shape, chunk, kind = case
    if name not in _cache:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        if kind == "embed":       # the source volume, extended along x
            src = volume(BY_NAME[_EMBED[name]])
            fill = _denoised(rng, shape[:2] + (shape[2] - src.shape[2],), dtype)
            a = np.concatenate([src, fill], axis=2)
        else:
            a = _KINDS[kind](rng, shape, dtype)
        assert a.dtype == dtype and a.shape == tuple(shape)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        _cache[name] = a
    return _cache[name]


def oracle_streams(case, version=2):
    """The oracle's stream of every chunk of the case, in (z, y, x) raster order (cached)."""
    key = (case[0], version)
    if key not in _cache:
        _cache[key] = [co.encode(c, version=version) for c in co.chunks(volume(case), case[3])]
    return _cache[key]


def chunk_index_map(src, dst):
    """Pairs (chunk of src, chunk of dst) of the same (bz, by, bx), for a dst that extends src along x."""
    gs = [-(-s // min(c, s)) for s, c in zip(src[2], src[3])]
    gd = [-(-s // min(c, s)) for s, c in zip(dst[2], dst[3])]
    assert gs[:2] == gd[:2] and gd[2] >= gs[2]
    return [((bz * gs[1] + by) * gs[2] + bx, (bz * gd[1] + by) * gd[2] + bx)
            for bz in range(gs[0]) for by in range(gs[1]) for bx in range(gs[2])]
