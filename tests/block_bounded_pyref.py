"""CPU restatement of the error-bounded chunk codec with a step per 8^3 block and a per-voxel bound (DESIGN.md 3.10c,
format "EB" version 1), built only from the oracle's transform quantiser (``oracle/bm4d_oracle.py``: ``dctq_forward``,
``dctq_inverse``), its EXAC coder (``oracle/codec_oracle.py``: ``encode``, ``decode``) and what ``bounded_pyref``
already offers.  Test infrastructure only."""
import struct

import numpy as np

from bounded_pyref import LADDER, STEPS, chunk_indices, chunk_slices, grid, reconstruct
from oracle import bm4d_oracle, codec_oracle

VERBATIM, OUTSIDE = 0xFE, 0xFF
__all__ = ["LADDER", "STEPS", "VERBATIM", "OUTSIDE", "grid", "chunk_slices", "header", "plane_bytes", "bounds",
           "choose_blocks", "volume_steps", "encode_chunk", "encode_volume", "decode_chunk"]


def header(mode, extent, chunk):
    return b"EB" + bytes((1, mode)) + bytes(8) + struct.pack("<6H", *extent, *chunk) + bytes(8)


def plane_bytes(chunk):
    nb = (chunk[0] // 8) * (chunk[1] // 8) * (chunk[2] // 8)
    return -(-nb // 16) * 16


def bounds(shape, delta, delta_fg=None, mask=None):
    """b(v): int64 array of ``shape``."""
    if mask is None:
        return np.full(shape, delta, dtype=np.int64)
    return np.where(np.asarray(mask) != 0, delta if delta_fg is None else delta_fg, delta).astype(np.int64)


def _per_block(a, lb, fill):
    """(ez, ey, ex) array -> (lbz, lby, lbx, 8, 8, 8) view of its blocks, the overhang holding ``fill``."""
    p = np.full(tuple(8 * n for n in lb), fill, dtype=a.dtype)
    p[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return p.reshape(lb[0], 8, lb[1], 8, lb[2], 8).transpose(0, 2, 4, 1, 3, 5)


def choose_blocks(vc, chunk, bc):
    """The block decisions of one chunk ``vc`` (its extent) under per-voxel bounds ``bc``, whatever mode the chunk
    ends up in -> (int16 steps over the nominal grid (cbz, cby, cbx) with -1 verbatim / -2 outside, int32 indices
    (cbz, cby, cbx, 512), reconstruction of the extent)."""
    vc = np.ascontiguousarray(vc)
    extent = vc.shape
    cb = tuple(c // 8 for c in chunk)
    lb = tuple(-(-e // 8) for e in extent)
    ref = vc.astype(np.int64)
    steps = np.full(cb, -2, dtype=np.int16)
    steps[:lb[0], :lb[1], :lb[2]] = -1
    inside = steps[:lb[0], :lb[1], :lb[2]]                      # a view: -1 = no verdict yet
    idx = np.zeros(cb + (512,), dtype=np.int32)
    rec = np.zeros(lb + (8, 8, 8), dtype=np.uint16)
    for j in range(STEPS - 1, -1, -1):                          # the first admissible step on the way down is max A
        if not np.any(inside == -1):
            break
        f = chunk_indices(vc, chunk, LADDER[j])
        r = reconstruct(f, extent, LADDER[j])
        excess = _per_block(np.abs(r.astype(np.int64) - ref) - bc, lb, np.int64(-1))
        take = (excess.reshape(lb + (512,)).max(axis=-1) <= 0) & (inside == -1)
        inside[take] = j
        idx[:lb[0], :lb[1], :lb[2]][take] = f[:lb[0], :lb[1], :lb[2]][take]
        rec[take] = _per_block(r, lb, np.uint16(0))[take]
    verb = inside == -1
    if np.any(verb):
        # the quantiser's edge replication: coordinates clamped to the chunk's extent
        z, y, x = (np.minimum(np.arange(8 * n), e - 1) for n, e in zip(lb, extent))
        rep = vc[np.ix_(z, y, x)]
        blocks = _per_block(rep, lb, np.uint16(0))
        idx[:lb[0], :lb[1], :lb[2]][verb] = blocks[verb].reshape(-1, 512).astype(np.int32)
        rec[verb] = blocks[verb]
    recon = rec.transpose(0, 3, 1, 4, 2, 5).reshape(tuple(8 * n for n in lb))[:extent[0], :extent[1], :extent[2]]
    return steps, idx, np.ascontiguousarray(recon)


def volume_steps(vol, chunk, delta, delta_fg=None, mask=None):
    """-> per chunk the (cbz, cby, cbx) int16 steps of ``choose_blocks`` (mode-0 chunks included)."""
    b = bounds(vol.shape, delta, delta_fg, mask)
    return [choose_blocks(vol[s], chunk, b[s])[0] for s in chunk_slices(vol.shape, chunk)]


def encode_chunk(vc, chunk, bc):
    """One chunk ``vc`` (its extent) with per-voxel bounds ``bc`` -> (stream bytes, reconstruction, int16 step plane
    [nb] with -1 verbatim / -2 outside, or None for a mode-0 chunk)."""
    vc = np.ascontiguousarray(vc)
    steps, idx, recon = choose_blocks(vc, chunk, bc)
    nb = steps.size
    plane = np.zeros(plane_bytes(chunk), dtype=np.uint8)
    flat = steps.reshape(-1)
    plane[:nb] = np.where(flat == -2, OUTSIDE, np.where(flat == -1, VERBATIM, flat)).astype(np.uint8)
    blocks_stream = plane.tobytes() + codec_oracle.encode(idx.reshape(nb, 8, 64))
    lossless = codec_oracle.encode(vc)
    if len(blocks_stream) < len(lossless):
        return header(1, vc.shape, chunk) + blocks_stream, recon, flat.copy()
    return header(0, vc.shape, chunk) + lossless, vc.copy(), None


def encode_volume(vol, chunk, delta, delta_fg=None, mask=None):
    """-> (list of chunk streams, reconstructed volume, list of step planes (None for a mode-0 chunk))."""
    b = bounds(vol.shape, delta, delta_fg, mask)
    streams, planes = [], []
    rec = np.empty_like(vol)
    for s in chunk_slices(vol.shape, chunk):
        blob, r, p = encode_chunk(vol[s], chunk, b[s])
        streams.append(blob)
        planes.append(p)
        rec[s] = r
    return streams, rec, planes


def decode_chunk(blob):
    """One chunk stream -> uint16 array of its extent; ValueError for a malformed stream."""
    raw = bytes(blob)
    if len(raw) <= 32 or raw[:2] != b"EB" or raw[2] != 1 or raw[3] not in (0, 1):
        raise ValueError("bad header")
    if raw[4:12] != bytes(8) or raw[24:32] != bytes(8):
        raise ValueError("reserved bytes")
    dims = struct.unpack("<6H", raw[12:24])
    extent, chunk = dims[:3], dims[3:]
    if any(c % 8 or c < 8 for c in chunk) or any(e < 1 or e > c for e, c in zip(extent, chunk)):
        raise ValueError("bad shapes")
    if raw[3] == 0:
        out, _ = codec_oracle.decode(raw[32:], int(np.prod(extent)), 2)
        return out.reshape(extent)
    cb = tuple(c // 8 for c in chunk)
    lb = tuple(-(-e // 8) for e in extent)
    nb, nbp = cb[0] * cb[1] * cb[2], plane_bytes(chunk)
    if len(raw) < 32 + nbp:
        raise ValueError("truncated plane")
    plane = np.frombuffer(raw[32:32 + nbp], dtype=np.uint8)
    if np.any(plane[nb:]):
        raise ValueError("plane padding")
    steps = plane[:nb].reshape(cb)
    idx, _ = codec_oracle.decode(raw[32 + nbp:], nb * 512, 4)
    idx = idx.reshape(cb + (512,))
    out = np.zeros(tuple(8 * n for n in lb), dtype=np.uint16)
    for bz in range(cb[0]):
        for by in range(cb[1]):
            for bx in range(cb[2]):
                s = int(steps[bz, by, bx])
                if bz >= lb[0] or by >= lb[1] or bx >= lb[2]:
                    if s != OUTSIDE:
                        raise ValueError("a block outside the volume carries a step")
                    continue
                ext = tuple(min(8, e - 8 * b) for e, b in zip(extent, (bz, by, bx)))
                dst = out[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
                if s == VERBATIM:
                    blk = idx[bz, by, bx].reshape(8, 8, 8)
                    part = blk[:ext[0], :ext[1], :ext[2]]
                    if part.min() < 0 or part.max() > 65535:
                        raise ValueError("a verbatim value is no voxel")
                    dst[:ext[0], :ext[1], :ext[2]] = part
                elif s < STEPS:
                    dst[:ext[0], :ext[1], :ext[2]] = bm4d_oracle.dctq_inverse(
                        np.ascontiguousarray(idx[bz:bz + 1, by:by + 1, bx:bx + 1]), ext, LADDER[s])
                else:
                    raise ValueError("a step beyond the ladder")
    return np.ascontiguousarray(out[:extent[0], :extent[1], :extent[2]])
