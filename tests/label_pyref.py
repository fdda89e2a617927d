"""numpy restatement of the label chunk format ``exac-labels`` version 1: what the GPU coder's bytes
are compared with.  One chunk at a time, no device, nothing shared with the package's own host code."""
import struct

import numpy as np

MAGIC = b"EXLB"
HEADER = 32
DTYPES = {4: np.dtype("<u4"), 8: np.dtype("<u8")}


def bits_of(k):
    """Index bits of a palette of ``k`` entries; None past 256 (a raw block)."""
    for most, bits in ((1, 0), (2, 1), (4, 2), (16, 4), (256, 8)):
        if k <= most:
            return bits
    return None


def _blocks(extent):
    return tuple(-(-e // 8) for e in extent)


def encode(chunk):
    """(z, y, x) uint32 / uint64 chunk -> its one valid stream."""
    a = np.ascontiguousarray(chunk)
    if a.ndim != 3 or a.size == 0 or a.dtype.itemsize not in DTYPES or a.dtype.kind != "u":
        raise ValueError("a chunk is a non-empty (z, y, x) array of uint32 or uint64")
    ts = a.dtype.itemsize
    nb = _blocks(a.shape)
    entries, payloads = [], []
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                sub = a[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
                values = np.unique(sub)                     # ascending, of the voxels present
                bits = bits_of(len(values))
                full = np.zeros((8, 8, 8), dtype=DTYPES[ts])
                if bits is None:
                    full[:sub.shape[0], :sub.shape[1], :sub.shape[2]] = sub
                    entries.append((0, 8 * ts))
                    payloads.append(full.tobytes())
                    continue
                palette = values.astype(DTYPES[ts]).tobytes()
                palette += bytes(-len(palette) % 8)
                index = np.zeros((8, 8, 8), dtype=np.uint64)    # absent slots hold index 0
                index[:sub.shape[0], :sub.shape[1], :sub.shape[2]] = np.searchsorted(values, sub)
                rows = index.reshape(64, 8)
                words = np.zeros(64, dtype=np.uint64)
                for x in range(8):
                    words |= rows[:, x] << np.uint64(x * bits)
                packed = words.astype("<u8").view(np.uint8).reshape(64, 8)[:, :bits].tobytes()
                entries.append((len(values), bits))
                payloads.append(palette + packed)
    at = (HEADER + 8 * len(entries)) // 8
    table = b""
    for (k, bits), payload in zip(entries, payloads):
        table += struct.pack("<IHBB", at, k, bits, 0)
        at += len(payload) // 8
    header = MAGIC + struct.pack("<HHIIIIII", 1, ts, a.shape[0], a.shape[1], a.shape[2], len(entries), 8 * at, 0)
    return header + table + b"".join(payloads)


def table(buf):
    """(offset in 8-byte units, k, bits) of every block of a stream, as three arrays; no checks."""
    n = struct.unpack_from("<I", buf, 20)[0]
    t = np.frombuffer(buf, dtype=np.dtype([("at", "<u4"), ("k", "<u2"), ("bits", "u1"), ("zero", "u1")]),
                      count=n, offset=HEADER)
    return t["at"].astype(np.int64), t["k"].astype(np.int64), t["bits"].astype(np.int64)


def validate(buf, typesize=None, extent=None):
    """``(typesize, extent)`` of a well-formed stream; ``ValueError`` for anything else.  ``typesize`` / ``extent``:
    what the reader expects, if it does."""
    buf = bytes(buf)
    if len(buf) < HEADER:
        raise ValueError("truncated stream: no header")
    if buf[:4] != MAGIC:
        raise ValueError("wrong magic")
    version, ts, ez, ey, ex, nblocks, total, zero = struct.unpack_from("<HHIIIIII", buf, 4)
    if version != 1:
        raise ValueError("wrong version")
    if ts not in DTYPES or (typesize is not None and ts != typesize):
        raise ValueError("wrong typesize")
    if min(ez, ey, ex) < 1 or (extent is not None and (ez, ey, ex) != tuple(extent)):
        raise ValueError("wrong extent")
    if nblocks != int(np.prod(_blocks((ez, ey, ex)))) or zero != 0:
        raise ValueError("wrong block count")
    if total != len(buf):
        raise ValueError("wrong total, or a truncated stream")
    if total < HEADER + 8 * nblocks or total % 8:
        raise ValueError("the table does not fit the stream")
    at, k, bits = table(buf)
    raw = bits == 8 * ts
    wanted = np.array([bits_of(int(v)) if 1 <= v <= 256 else -1 for v in k], dtype=np.int64)
    if np.any(raw & (k != 0)) or np.any(~raw & (bits != wanted)):
        raise ValueError("a block's k disagrees with its bits")
    size = np.where(raw, 512 * ts, (k * ts + 7) // 8 * 8 + 64 * bits)
    if np.any(8 * at + size > total):
        raise ValueError("a table offset past the end of the stream")
    if np.any(np.diff(at) <= 0):
        raise ValueError("table offsets are not ascending")
    begin = np.concatenate(([(HEADER + 8 * nblocks) // 8], (at + size // 8)[:-1]))
    if np.any(at != begin) or 8 * int(at[-1]) + int(size[-1]) != total:
        raise ValueError("payloads are not contiguous in block order")
    return ts, (ez, ey, ex)


def decode(buf):
    """A valid stream -> its (z, y, x) chunk."""
    ts, extent = validate(buf)
    buf = bytes(buf)
    at, k, bits = table(buf)
    nb = _blocks(extent)
    out = np.zeros(tuple(8 * n for n in nb), dtype=DTYPES[ts])
    b = 0
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                p = 8 * int(at[b])
                if bits[b] == 8 * ts:
                    block = np.frombuffer(buf, dtype=DTYPES[ts], count=512, offset=p)
                else:
                    palette = np.frombuffer(buf, dtype=DTYPES[ts], count=int(k[b]), offset=p)
                    index = np.zeros(512, dtype=np.int64)
                    if bits[b]:
                        p += (int(k[b]) * ts + 7) // 8 * 8
                        stream = np.unpackbits(np.frombuffer(buf, dtype=np.uint8, count=64 * int(bits[b]), offset=p),
                                               bitorder="little").reshape(512, int(bits[b])).astype(np.int64)
                        index = (stream << np.arange(int(bits[b]))).sum(axis=1)
                    if index.max() >= k[b]:
                        raise ValueError("a palette index outside its palette")
                    block = palette[index]
                out[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = block.reshape(8, 8, 8)
                b += 1
    return np.ascontiguousarray(out[:extent[0], :extent[1], :extent[2]])


CLASS_COUNTS = (1, 2, 3, 4, 5, 16, 17, 256, 257, 512)


def class_volume(shape=(40, 24, 19), dtype=np.uint64, seed=7, counts=CLASS_COUNTS):
    """A volume over a zero background whose first 8^3 blocks (anchored at multiples of 8, which chunks of a multiple
    of 8 keep) hold exactly ``counts`` distinct values each -- by default both sides of every class boundary -- with
    the ids 0, 2^32 - 1 and (uint64) 2^32, 2^64 - 1 among them.  Where x is no multiple of 8, two of the truncated
    blocks there hold 3 and 20 values."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    big = [0, 2 ** 32 - 1] + ([2 ** 32, 2 ** 64 - 1] if dt.itemsize == 8 else [2 ** 31, 2 ** 32 - 2])
    pool = np.array(big + [int(v) for v in rng.choice(np.arange(1000, 5000), 600, replace=False) * 3 + 1],
                    dtype=np.uint64).astype(dt)
    vol = np.zeros(shape, dtype=dt)
    spots = [(z, y, x) for z in range(0, shape[0] - 7, 8) for y in range(0, shape[1] - 7, 8)
             for x in range(0, shape[2] - 7, 8)]
    assert len(spots) >= len(counts)
    for n, (z, y, x) in zip(counts, spots):
        ids = np.concatenate([pool[:n], rng.choice(pool[:n], 512 - n)])
        vol[z:z + 8, y:y + 8, x:x + 8] = rng.permutation(ids).reshape(8, 8, 8)
    # the truncated blocks along x (3 wide): 3 values in one, 20 in another
    x0 = shape[2] // 8 * 8
    if x0 < shape[2]:
        w = shape[2] - x0
        vol[0:8, 0:8, x0:] = rng.permutation(np.resize(pool[:3], 64 * w)).reshape(8, 8, w)
        vol[8:16, 8:16, x0:] = rng.permutation(np.resize(pool[:20], 64 * w)).reshape(8, 8, w)
    return vol


def tube_volume(shape=(64, 64, 64), dtype=np.uint64, seed=3):
    """Tubes and blobs with large ids over a zero background, plus a speckled corner."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij")
    vol = np.zeros(shape, dtype=dt)
    top = 2 ** (8 * dt.itemsize) - 1
    for i in range(6):
        c = rng.uniform(0.2, 0.8, 2) * np.array(shape[1:])
        r = rng.uniform(2.0, 5.0)
        wob = 3.0 * np.sin(z / 7.0 + i)
        vol[(y - c[0] - wob) ** 2 + (x - c[1] + wob) ** 2 < r * r] = top - 1000 * i
    for i in range(4):
        c = rng.uniform(0.1, 0.9, 3) * np.array(shape)
        r = rng.uniform(3.0, 8.0)
        vol[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 < r * r] = 2 ** 32 // 3 + i
    s = tuple(max(1, n // 4) for n in shape)
    vol[:s[0], :s[1], :s[2]] = rng.integers(1, 400, s).astype(dt)
    return vol
