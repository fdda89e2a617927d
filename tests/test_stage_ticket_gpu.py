"""The stage kernels hand their groups out by ticket: which pair of waves transforms which
group depends on timing, the sums are integers, so the uint16 volume must be the CPU oracle's bit for bit
whatever the launch shape -- one z chunk or three, tile columns in raster order or in strips -- and the same
again on a second call.

Shapes (planes, rows, columns; a grid point every 4 voxels and one at the end):
  16 x 12 x 12   one tile of 2 x 2 groups, fewer groups than wave pairs in both kernels; 3 layers
  40 x 12 x 20   exactly one full 2 x 4 tile; 9 layers: the tickets wrap the eight report-counter slots
  40 x 16 x 24   3 x 5 grid points: a full tile next to partial ones in both directions; 9 layers
  45 x 30 x 37   ragged on every axis, the last grid point off the multiple of 4
  72 x 24 x 40   values constant per 8^3 block (float32 levels, stored as counts): far fewer matches, so
                 many groups of one and two blocks -- the idle second wave of a pair
"""
import functools

import numpy as np
import pytest

from util import synth_volume

pytestmark = pytest.mark.gpu

SIGMA, OFFSET = 24.0, 37.0


def block_constant_volume(shape, seed):
    """uint16 counts whose float32 values are constant on every 8^3 block, twelve levels 40 counts apart: a
    block matches a shifted copy of itself only where the neighbouring levels are close, so the group sizes
    spread from one block to the full sixteen."""
    rng = np.random.default_rng(seed)
    nb = [-(-n // 8) for n in shape]
    levels = (OFFSET + 40.0 * rng.integers(0, 12, size=nb)).astype(np.float32)
    vol = np.repeat(np.repeat(np.repeat(levels, 8, 0), 8, 1), 8, 2)[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(vol).astype(np.uint16)


CASES = {
    "one_tile_2x2": lambda: synth_volume((16, 12, 12), seed=31, as_u16=True)[0],
    "one_full_tile_9_layers": lambda: synth_volume((40, 12, 20), seed=32, as_u16=True)[0],
    "tiles_3x5_9_layers": lambda: synth_volume((40, 16, 24), seed=33, as_u16=True)[0],
    "ragged": lambda: synth_volume((45, 30, 37), seed=34, as_u16=True)[0],
    "block_constant": lambda: block_constant_volume((72, 24, 40), 35),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, the oracle's uint16 result), computed once and read-only."""
    from oracle import bm4d_oracle
    bm4d_oracle.build()
    vol = CASES[name]()
    want = bm4d_oracle.bm4d_u16(vol, SIGMA, OFFSET)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def test_block_constant_case_has_small_groups(oracle):
    """The fifth case is there for groups of one and two blocks, in the tables of both stages."""
    vol, _ = case("block_constant")
    counts = vol.astype(np.float32) - np.float32(OFFSET)
    basic = oracle.bm4d(counts, SIGMA, stages=1)
    for keys in (oracle.blockmatch(counts, SIGMA), oracle.blockmatch(basic, SIGMA, 0.6)):
        size = (keys.reshape(-1, 16) != 0xFFFFFFFF).sum(axis=1)
        assert (size == 1).sum() >= 20 and ((size == 2) | (size == 3)).sum() >= 20, np.bincount(size, minlength=17)


@pytest.mark.parametrize("name", list(CASES))
def test_every_launch_shape_gives_the_oracles_volume(ctx, name):
    vol, want = case(name)
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
                assert np.array_equal(got, want), (
                    f"stage_chunks {chunks}, stage_strip {strip}: {np.count_nonzero(got != want)} voxels differ")
    finally:
        ctx.set_option("stage_chunks", 0)
        ctx.set_option("stage_strip", 3)
        d_in.free()
        d_out.free()


def test_second_call_on_the_same_context_is_identical(ctx):
    vol, want = case("ragged")
    d_in = ctx.to_device(vol)
    d_out = ctx.alloc(vol.nbytes)
    try:
        runs = []
        for _ in range(2):
            d_out.fill(0xA5)
            ctx.denoise_u16(d_in, d_out, vol.shape, SIGMA, OFFSET)
            ctx.sync()
            runs.append(d_out.download(vol.shape, np.uint16))
        assert np.array_equal(runs[0], runs[1])
        assert np.array_equal(runs[0], want)
    finally:
        d_in.free()
        d_out.free()
