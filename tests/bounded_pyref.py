"""CPU restatement of the error-bounded lossy chunk codec, built only from the oracle's
transform quantiser (``oracle/bm4d_oracle.py``: ``dctq_forward``, ``dctq_inverse``) and EXAC coder
(``oracle/codec_oracle.py``: ``encode``, ``decode``).  Test infrastructure only."""
import struct

import numpy as np

from oracle import bm4d_oracle, codec_oracle

STEPS = 29
LADDER = np.array([np.float32(2.0 ** ((j - 4) / 4)) for j in range(STEPS)], dtype=np.float32)


def grid(shape, chunk):
    return tuple(-(-s // c) for s, c in zip(shape, chunk))


def chunk_slices(shape, chunk):
    """(z, y, x) raster of chunk slices, edge chunks truncated."""
    g = grid(shape, chunk)
    for iz in range(g[0]):
        for iy in range(g[1]):
            for ix in range(g[2]):
                yield tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip((iz, iy, ix), chunk, shape))


def header(mode, j, extent, chunk):
    q = float(LADDER[j]) if mode == 1 else 0.0
    return (b"EQ" + bytes((1, mode, 0xFF if mode == 0 else j, 0, 0, 0)) + struct.pack("<f", q)
            + struct.pack("<6H", *extent, *chunk) + bytes(8))


def chunk_indices(vc, chunk, q):
    """The chunk's indices over its nominal block grid (nb, 8, 64): dctq_forward of the chunk in the leading
    ceil(E/8) blocks, zeros elsewhere."""
    idx = np.zeros(tuple(c // 8 for c in chunk) + (512,), dtype=np.int32)
    f = bm4d_oracle.dctq_forward(vc, q)
    idx[:f.shape[0], :f.shape[1], :f.shape[2]] = f
    return idx


def reconstruct(idx, extent, q):
    lb = tuple(-(-e // 8) for e in extent)
    return bm4d_oracle.dctq_inverse(np.ascontiguousarray(idx[:lb[0], :lb[1], :lb[2]]), extent, q)


def ladder_errors(vc, chunk):
    """err_j of one chunk for every step."""
    err = np.zeros(STEPS, dtype=np.uint32)
    ref = vc.astype(np.int64)
    for j in range(STEPS):
        r = reconstruct(chunk_indices(vc, chunk, LADDER[j]), vc.shape, LADDER[j])
        err[j] = int(np.abs(r.astype(np.int64) - ref).max())
    return err


def volume_ladder(vol, chunk):
    """uint32 [gz, gy, gx, 29]."""
    g = grid(vol.shape, chunk)
    return np.stack([ladder_errors(np.ascontiguousarray(vol[s]), chunk)
                     for s in chunk_slices(vol.shape, chunk)]).reshape(g + (STEPS,))


def encode_chunk(vc, chunk, delta, err=None):
    """-> (stream bytes, reconstruction, j* or None for a lossless chunk)."""
    vc = np.ascontiguousarray(vc)
    err = ladder_errors(vc, chunk) if err is None else err
    admissible = [j for j in range(STEPS) if err[j] <= delta]
    lossless = codec_oracle.encode(vc)
    if admissible:
        j = max(admissible)
        idx = chunk_indices(vc, chunk, LADDER[j])
        nb = idx.shape[0] * idx.shape[1] * idx.shape[2]
        lossy = codec_oracle.encode(idx.reshape(nb, 8, 64))
        if len(lossy) < len(lossless):
            return header(1, j, vc.shape, chunk) + lossy, reconstruct(idx, vc.shape, LADDER[j]), j
    return header(0, 0, vc.shape, chunk) + lossless, vc.copy(), None


def encode_volume(vol, chunk, delta, errs=None):
    """-> (list of chunk streams, reconstructed volume, list of j* per chunk)."""
    errs = volume_ladder(vol, chunk) if errs is None else errs
    errs = errs.reshape(-1, STEPS)
    streams, steps = [], []
    rec = np.empty_like(vol)
    for k, s in enumerate(chunk_slices(vol.shape, chunk)):
        blob, r, j = encode_chunk(vol[s], chunk, delta, errs[k])
        streams.append(blob)
        steps.append(j)
        rec[s] = r
    return streams, rec, steps


def decode_chunk(blob):
    """One chunk stream -> uint16 array of its extent; ValueError for a malformed stream."""
    raw = bytes(blob)
    if len(raw) <= 32 or raw[:2] != b"EQ" or raw[2] != 1 or raw[3] not in (0, 1):
        raise ValueError("bad header")
    mode, j = raw[3], raw[4]
    q = struct.unpack("<f", raw[8:12])[0]
    dims = struct.unpack("<6H", raw[12:24])
    extent, chunk = dims[:3], dims[3:]
    if any(c % 8 or c < 8 for c in chunk) or any(e < 1 or e > c for e, c in zip(extent, chunk)):
        raise ValueError("bad shapes")
    n = int(np.prod(extent))
    if mode == 0:
        if j != 0xFF or q != 0.0:
            raise ValueError("bad lossless header")
        out, _ = codec_oracle.decode(raw[32:], n, 2)
        return out.reshape(extent)
    if j >= STEPS or np.float32(q) != LADDER[j]:
        raise ValueError("bad step")
    nb = (chunk[0] // 8) * (chunk[1] // 8) * (chunk[2] // 8)
    idx, _ = codec_oracle.decode(raw[32:], nb * 512, 4)
    return reconstruct(idx.reshape(chunk[0] // 8, chunk[1] // 8, chunk[2] // 8, 512), extent, LADDER[j])
