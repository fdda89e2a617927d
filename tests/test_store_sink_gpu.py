"""``store_windows.BrickSink``, the write side that the store-to-store operators share: bricks written
through it from device buffers are, chunk file for chunk file, ``write_zarr`` of the volume; a brick that leaves a chunk
uncovered is refused before a file exists; and whatever ends the block, nothing stays allocated.

One volume of 20 x 24 x 40 in chunks of 8 x 16 x 16: three chunks along every axis, the last one cut on each."""
import os

import numpy as np
import pytest

from aind_exaspim_image_compression.utils import chunk_store, store_windows, store_write
from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec

pytestmark = pytest.mark.gpu

SHAPE = (20, 24, 40)
CHUNKS = (1, 1, 8, 16, 16)
BRICKS = (((0, 0, 0), (16, 24, 40)), ((16, 0, 0), (4, 24, 40)))       # z [0, 16) and [16, 20)
PLANE = SHAPE[1] * SHAPE[2]


def _files(path):
    out = {}
    for dirpath, _, names in os.walk(path):
        for name in names:
            with open(os.path.join(dirpath, name), "rb") as f:
                out[os.path.relpath(os.path.join(dirpath, name), path)] = f.read()
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The volume and the files ``write_zarr`` makes of it."""
    vol = np.random.default_rng(3).poisson(120, SHAPE).astype(np.uint16)
    vol[5:9, 10:20, 14:34] += 3000
    whole = str(tmp_path_factory.mktemp("sink") / "whole")
    chunk_store.write_zarr(vol, whole, CHUNKS, codec=ExacCodec(2))
    vol.setflags(write=False)
    return vol, _files(whole)


def _new_store(path, codec=None):
    return chunk_store.create_zarr(str(path), SHAPE, CHUNKS, codec=codec or ExacCodec(2), overwrite=True, device=0)


def test_bricks_from_a_device_buffer_are_write_zarr_of_the_volume(ctx, case, tmp_path):
    vol, want = case
    out = _new_store(tmp_path / "dst")
    with ctx.to_device(vol) as d_vol, store_windows.BrickSink("sink_test", out, ctx, SHAPE, CHUNKS) as sink:
        for origin, extent in BRICKS:
            with sink.pool([origin], [extent]) as pool:
                assert len(pool.g.chunks) == -(-extent[0] // 8) * 2 * 3
                # the brick is whole layers of the volume: the box's own strides, from its first layer on
                records = store_write.box_records([origin], extent, base=origin[0] * PLANE)
                pool.scatter(d_vol, vol.size, np.uint16, records)
                pool.commit()
    got = _files(out.path)
    assert sorted(got) == sorted(want) and got == want
    assert sink.written == sum(len(b) for name, b in got.items() if name != "zarr.json")
    seconds = {}
    assert sink.finish(seconds) == {"chunks": 3 * 2 * 3, "encode_calls": sink.st["encode_calls"]}
    assert set(seconds) == {"encode", "files_write"} and sink.st["encode_calls"] >= 2


def test_a_box_that_leaves_a_chunk_uncovered_is_refused_before_any_file(ctx, case, tmp_path):
    out = _new_store(tmp_path / "dst")
    with store_windows.BrickSink("sink_test", out, ctx, SHAPE, CHUNKS) as sink:
        with pytest.raises(RuntimeError, match="sink_test"):
            with sink.pool([(0, 0, 0)], [(8, 16, 10)]):                # 10 of the chunk's 16 voxels along x
                raise AssertionError("the pool was opened")
    assert sink.written == 0 and list(_files(out.path)) == ["zarr.json"]


def test_an_exception_inside_the_pool_block_propagates_and_frees_everything(ctx, case, tmp_path, monkeypatch):
    vol, _ = case
    codec = BlockBoundedCodec.from_noise({"gain": 1.0, "read_noise": 2.0, "offset": 100.0}, k=0.5, max_error=40,
                                         fg_max_error=1)
    assert codec.bound_table is not None
    out = _new_store(tmp_path / "dst", codec)
    handed_out = []
    for name in ("alloc", "to_device"):
        def recording(*a, _inner=getattr(ctx, name), **k):
            handed_out.append(_inner(*a, **k))
            return handed_out[-1]
        monkeypatch.setattr(ctx, name, recording)

    class Stop(Exception):
        pass

    with pytest.raises(Stop):
        with store_windows.BrickSink("sink_test", out, ctx, SHAPE, CHUNKS) as sink:
            origin, extent = BRICKS[0]
            with sink.pool([origin], [extent], want_mask=True) as pool:
                d_vol = ctx.to_device(vol)
                pool.scatter(d_vol, vol.size, np.uint16, store_write.box_records([origin], extent))
                assert pool.pool.mask is not None and sink.d_table is not None
                d_vol.free()
                raise Stop()
    assert len(handed_out) == 4                                        # the table, the pool, the mask pool, the volume
    assert all(buf.ptr is None for buf in handed_out)
    assert sink.written == 0 and list(_files(out.path)) == ["zarr.json"]


def test_one_group_of_two_boxes_scattered_one_by_one_as_denoise_store_does(ctx, case, tmp_path):
    vol, want = case
    out = _new_store(tmp_path / "dst")
    with store_windows.BrickSink("sink_test", out, ctx, SHAPE, CHUNKS, box="core") as sink:
        with sink.pool([o for o, _ in BRICKS], [e for _, e in BRICKS]) as pool:
            assert len(pool.g.chunks) == 3 * 2 * 3
            for k, (origin, extent) in enumerate(BRICKS):
                # a buffer that holds box k alone: the group's lists in terms of this one record
                part = np.ascontiguousarray(vol[origin[0]:origin[0] + extent[0]])
                remap = np.full(len(BRICKS) + 1, -1, dtype=np.int32)              # [-1] stays -1
                remap[k] = 0
                with ctx.to_device(part) as d_part:
                    pool.scatter(d_part, part.size, np.uint16, store_write.box_records([origin], extent),
                                 dst_boxes=remap[pool.g.dst_boxes])
                    ctx.sync()
            pool.commit()
    got = _files(out.path)
    assert got == want and sink.st["groups"] == 1
    assert sink.written == sum(len(b) for name, b in got.items() if name != "zarr.json")
