"""CPU restatement of the block-bounded codec with a bound table: the bound of a voxel is
``b(v) = min(T[V(v)], where(mask, fg_max_error, max_error))`` with ``T`` a table of 65536 uint16 indexed by the voxel's
own value.  Everything else -- block decisions, modes, the "EB" version 1 stream -- is ``block_bounded_pyref``'s, used
as it is.  Also the volumes the table tests share.  Test infrastructure only."""
import numpy as np

import block_bounded_pyref as base
from block_bounded_pyref import chunk_slices, choose_blocks, decode_chunk, encode_chunk, grid

__all__ = ["bounds", "volume_steps", "encode_volume", "decode_chunk", "chunk_slices", "grid", "pg_volume", "MAIN",
           "NOISE", "formula_table"]

MAIN = ((21, 27, 43), (16, 16, 24))     # cbx = 3: a duplicate pair; outside blocks; ragged extents on all axes
NOISE = {"gain": 2.0, "read_noise": 3.0, "offset": 100.0}


def bounds(vol, delta, delta_fg=None, mask=None, table=None):
    """b(v): int64 array of ``vol.shape``; without a table ``block_bounded_pyref.bounds``."""
    b = base.bounds(vol.shape, delta, delta_fg, mask)
    if table is None:
        return b
    t = np.asarray(table)
    assert t.dtype == np.uint16 and t.shape == (65536,)
    return np.minimum(b, t[vol].astype(np.int64))


def volume_steps(vol, chunk, delta, delta_fg=None, mask=None, table=None):
    """-> per chunk the (cbz, cby, cbx) int16 steps of ``choose_blocks`` (mode-0 chunks included)."""
    b = bounds(vol, delta, delta_fg, mask, table)
    return [choose_blocks(vol[s], chunk, b[s])[0] for s in chunk_slices(vol.shape, chunk)]


def encode_volume(vol, chunk, delta, delta_fg=None, mask=None, table=None):
    """-> (list of chunk streams, reconstructed volume, list of step planes (None for a mode-0 chunk))."""
    b = bounds(vol, delta, delta_fg, mask, table)
    streams, planes = [], []
    rec = np.empty_like(vol)
    for s in chunk_slices(vol.shape, chunk):
        blob, r, p = encode_chunk(vol[s], chunk, b[s])
        streams.append(blob)
        planes.append(p)
        rec[s] = r
    return streams, rec, planes


def formula_table(noise, k, cap=65535):
    """The table of DESIGN.md 3.10d entry by entry with Python floats (IEEE float64): min(cap, floor(k sqrt(gain
    max(c - offset, 0) + read_noise^2)))."""
    import math
    return np.array([min(cap, math.floor(k * math.sqrt(noise["gain"] * max(c - noise["offset"], 0.0)
                                                       + noise["read_noise"] * noise["read_noise"])))
                     for c in range(65536)], dtype=np.uint16)


def pg_volume(shape, seed=11, special=True):
    """uint16 volume under the Poisson-Gaussian model ``NOISE``: a smooth ramp plus blobs from the pedestal (100) to
    about 20000 counts.  With ``special`` (shapes of at least (16, 16, 24)): the 8^3 block at (8, 8, 16) is a
    0 / 65535 checkerboard, and the block at (0, 8, 0) is dark except for one bright voxel."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    clean = 40.0 * (x / max(shape[2] - 1, 1)) + 25.0 * (y / max(shape[1] - 1, 1))
    for a in (20000.0, 8000.0, 3000.0, 1000.0):
        c = [rng.uniform(0.25 * n, 0.75 * n) for n in shape]
        r = rng.uniform(2.0, 5.0)
        clean += a * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2.0 * r * r))
    g, rn, off = NOISE["gain"], NOISE["read_noise"], NOISE["offset"]
    counts = g * rng.poisson(clean / g) + rng.normal(off, rn, shape)
    vol = np.rint(np.clip(counts, 0, 65535)).astype(np.uint16)
    if special:
        assert shape[0] >= 16 and shape[1] >= 16 and shape[2] >= 24
        cz, cy, cx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
        vol[8:16, 8:16, 16:24] = (((cz + cy + cx) & 1) * 65535).astype(np.uint16)
        vol[0:8, 8:16, 0:8] = np.rint(np.clip(rng.normal(off, rn, (8, 8, 8)), 0, 65535)).astype(np.uint16)
        vol[3, 12, 5] = 30000
    return vol
