"""The stage kernels flush a plane of the numerator ring with 64-bit global atomics whose address is a scalar
base per plane -- region element (0, 0), which lies before the array for tiles at the low edges -- plus a 32-bit
offset per lane that is stepped, not divided.  A mis-addressed or dropped flush row moves the
sums of some voxels, so the uint16 volume must be the CPU oracle's bit for bit at every launch shape.

Shapes (planes, rows, columns; a tile is 2 x 4 grid points, its ring region 22 x 30 voxels):
  16 x  9 x 11   one tile whose region lies mostly outside the volume: the origin is negative in y and x, the
                 volume's rows are shorter than the region's, so every region row wraps
  24 x 30 x 70   4 x 5 tiles: the region is inside the volume for the interior ones and cut on all four sides
                 for the rest; 70 columns are no multiple of a tile's 16
  45 x 13 x 37   ragged: the last grid point is off the multiple of 4 on every axis

Noise of sigma 64: the denoised count of a voxel then equals its input with a probability well below 1 %, so
every border face of the oracle's volume differs from the input on at least 99 % of its voxels, and a flush that
left a border row out would show there.
"""
import functools

import numpy as np
import pytest

from util import synth_volume

SIGMA, OFFSET = 64.0, 37.0

CASES = {
    "one_tile_negative_origin": ((16, 9, 11), 56),       # (its 99-voxel faces must differ on every voxel: the first seed that does)
    "tiles_4x5": ((24, 30, 70), 42),
    "ragged": ((45, 13, 37), 43),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, the oracle's uint16 result), computed once and read-only."""
    from oracle import bm4d_oracle
    bm4d_oracle.build()
    shape, seed = CASES[name]
    vol = synth_volume(shape, seed=seed, sigma=SIGMA, pedestal=OFFSET + 400.0, as_u16=True)[0]
    want = bm4d_oracle.bm4d_u16(vol, SIGMA, OFFSET)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def border_faces(a):
    return {"z0": a[0], "z1": a[-1], "y0": a[:, 0], "y1": a[:, -1], "x0": a[:, :, 0], "x1": a[:, :, -1]}


def changed_share_of_faces(vol, want):
    changed = border_faces(want != vol)
    return {k: float(np.mean(v)) for k, v in changed.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_changes_every_border_face(name):
    """On the oracle alone: each one-voxel-thick border face differs from the input on >= 99 % of its voxels."""
    vol, want = case(name)
    share = changed_share_of_faces(vol, want)
    print(name, share)
    assert min(share.values()) >= 0.99, share


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_flush_gives_the_oracles_volume_at_every_launch_shape(ctx, name):
    vol, want = case(name)
    share = changed_share_of_faces(vol, want)
    assert min(share.values()) >= 0.99, share
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    try:
        for chunks in (1, 3):
            for strip in (0, 3):
                ctx.set_option("stage_chunks", chunks)
                ctx.set_option("stage_strip", strip)
                d_out.fill(0xA5)
                ctx.denoise_u16(d_in, d_out, vol.shape, SIGMA, OFFSET)
                ctx.sync()
                got = d_out.download(vol.shape, np.uint16)
                diff = got != want
                assert not diff.any(), (
                    f"stage_chunks {chunks}, stage_strip {strip}: {np.count_nonzero(diff)} voxels differ, "
                    f"per border face {({k: int(v.sum()) for k, v in border_faces(diff).items()})}")
    finally:
        ctx.set_option("stage_chunks", 0)
        ctx.set_option("stage_strip", 3)
        d_in.free()
        d_out.free()
