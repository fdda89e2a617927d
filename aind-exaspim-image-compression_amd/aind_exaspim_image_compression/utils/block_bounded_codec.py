"""Error-bounded lossy chunk codec with a ladder step per 8^3 block and a per-voxel bound.

``BoundedDctCodec`` picks one quantiser step per chunk, so one bright structure sets the step of
all 512 blocks of a 64^3 chunk, and its bound is the same for every voxel.  Here every 8^3 block takes the coarsest
step of the same ladder whose reconstruction stays within the bound of each of ITS voxels, and the bound of a voxel
is ``fg_max_error`` where a caller-supplied mask is set and ``max_error`` elsewhere: neurites exact (or within one
count) and the background within eight is one stored array.  A block that no step satisfies is stored verbatim, and a
chunk whose block stream is not shorter than its lossless EXAC stream is stored as the latter, so the guarantee
``|decoded - input| <= bound`` holds for any mask and any ``fg_max_error <= max_error``.

With a ``bound_table`` the bound of a voxel is further capped by the table's entry at the voxel's own
value: ``b(v) = min(T[V(v)], where(mask, fg_max_error, max_error))``.  ``BlockBoundedCodec.from_noise(noise, k)`` makes
the table from measured Poisson-Gaussian parameters (``utils/noise.py``), so that no voxel is off by more than ``k``
noise standard deviations of its own intensity.  Only the encoder sees the table; streams and decoder are unchanged.

The format ("EB" version 1) is a sibling of the bounded codec's "EQ" version 1, with its own magic, codec id and
C-ABI entries; step choice, quantiser, both entropy coders, assembly and decode run on the MI355X
(``csrc/block_bounded_kernels.hip``, ``exabm4d_block_bounded_*``).
"""
import hashlib

import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils.bounded_codec import (HEADER_BYTES, LADDER, STEPS, BoundedVolumeCodec,
                                                                 pack_dims, parse_dims)
from aind_exaspim_image_compression.utils.chunk_codec import _shape3

FORMAT_VERSION = 1
MODE_LOSSLESS, MODE_BLOCKS = 0, 1
STEP_VERBATIM, STEP_OUTSIDE = 0xFE, 0xFF
__all__ = ["BlockBoundedCodec", "pack_header", "parse_header", "plane_bytes", "LADDER", "STEPS"]


def plane_bytes(chunk):
    """Bytes of a chunk's step plane: one per block of the nominal grid, padded to a multiple of 16."""
    nb = (int(chunk[0]) // 8) * (int(chunk[1]) // 8) * (int(chunk[2]) // 8)
    return -(-nb // 16) * 16


def pack_header(mode, extent, chunk):
    """The 32-byte header of a chunk stream (mode 0: lossless EXAC uint16 payload; mode 1: step plane, then the EXAC
    int32 stream of the block indices)."""
    h = bytearray(HEADER_BYTES)
    h[0:4] = bytes((ord("E"), ord("B"), FORMAT_VERSION, int(mode)))
    h[12:24] = pack_dims(extent, chunk)
    return bytes(h)


def _inside_blocks(extent, chunk):
    """bool [nb]: the blocks of the nominal grid, raster order, that hold a voxel of the chunk's extent."""
    cb = tuple(c // 8 for c in chunk)
    lb = tuple(-(-e // 8) for e in extent)
    z, y, x = np.meshgrid(*(np.arange(n) for n in cb), indexing="ij")
    return ((z < lb[0]) & (y < lb[1]) & (x < lb[2])).reshape(-1)


def parse_header(blob):
    """-> dict(mode, extent, chunk, steps) of a chunk stream.  ``steps`` is None for mode 0 and the int16 plane for
    mode 1 (-1 verbatim, -2 outside).  Everything that can be said about a stream without decoding its EXAC payload is
    checked here, on the host: ``ValueError`` for a bad magic, version or mode, a non-zero reserved byte, shapes
    outside ``1 <= E <= C`` with ``C`` a multiple of 8, a plane byte that is no step or 0xFE on an inside block or not
    0xFF on an outside one, non-zero plane padding, a payload whose EXAC header does not match mode, ``E`` and ``C``,
    and a stream too short for any of it."""
    raw = bytes(blob)
    if len(raw) <= HEADER_BYTES:
        raise ValueError("block-bounded chunk stream: truncated (no payload behind the 32-byte header)")
    if raw[0:2] != b"EB":
        raise ValueError("block-bounded chunk stream: bad magic")
    if raw[2] != FORMAT_VERSION:
        raise ValueError(f"block-bounded chunk stream: unknown format version {raw[2]}")
    mode = raw[3]
    if mode not in (MODE_LOSSLESS, MODE_BLOCKS):
        raise ValueError(f"block-bounded chunk stream: unknown mode {mode}")
    if raw[4:12] != bytes(8) or raw[24:32] != bytes(8):
        raise ValueError("block-bounded chunk stream: reserved header bytes are not zero")
    extent, chunk = parse_dims(raw, "block-bounded")
    steps, at = None, HEADER_BYTES
    if mode == MODE_BLOCKS:
        nb = (chunk[0] // 8) * (chunk[1] // 8) * (chunk[2] // 8)
        nbp = plane_bytes(chunk)
        if len(raw) < HEADER_BYTES + nbp:
            raise ValueError("block-bounded chunk stream: truncated step plane")
        plane = np.frombuffer(raw[at:at + nbp], dtype=np.uint8)
        inside = _inside_blocks(extent, chunk)
        if np.any(plane[nb:]):
            raise ValueError("block-bounded chunk stream: step plane padding is not zero")
        if np.any(plane[:nb][~inside] != STEP_OUTSIDE):
            raise ValueError("block-bounded chunk stream: a block outside the volume carries a step")
        if np.any((plane[:nb][inside] >= STEPS) & (plane[:nb][inside] != STEP_VERBATIM)):
            raise ValueError("block-bounded chunk stream: a step beyond the ladder")
        steps = plane[:nb].astype(np.int16)
        steps[plane[:nb] == STEP_VERBATIM] = -1
        steps[plane[:nb] == STEP_OUTSIDE] = -2
        at += nbp
        want = (4, nb * 512, 8, 64)
    else:
        want = (2, extent[0] * extent[1] * extent[2], extent[1], extent[2])
    if len(raw) < at + 16:
        raise ValueError("block-bounded chunk stream: truncated EXAC payload")
    got = (raw[at + 3],) + tuple(int(v) for v in np.frombuffer(raw[at + 4:at + 16], dtype="<u4"))
    if raw[at:at + 3] != b"EX\x02" or got != want:
        raise ValueError("block-bounded chunk stream: the EXAC payload does not match mode, extent and chunk")
    return {"mode": int(mode), "extent": extent, "chunk": chunk, "steps": steps}


class BlockBoundedCodec(BoundedVolumeCodec):
    """numcodecs-shaped codec of uint16 chunks with a per-voxel error bound and a step per 8^3 block, arithmetic on
    the GPU."""

    codec_id = "exac-dctq-block"
    version = FORMAT_VERSION
    noun = "block-bounded"
    takes_mask = True
    parse_header = staticmethod(parse_header)

    def __init__(self, max_error=65535, fg_max_error=None, bound_table=None, device=None):
        max_error = int(max_error)
        fg_max_error = max_error if fg_max_error is None else int(fg_max_error)
        if not 0 <= fg_max_error <= max_error <= 65535:
            raise ValueError("0 <= fg_max_error <= max_error <= 65535 is required")
        if bound_table is not None:
            if not isinstance(bound_table, np.ndarray) or bound_table.dtype != np.uint16 or \
                    bound_table.shape != (65536,):
                raise ValueError("bound_table must be a uint16 array of shape (65536,)")
            bound_table = np.ascontiguousarray(bound_table).copy()
            bound_table.setflags(write=False)
        self.max_error = max_error
        self.fg_max_error = fg_max_error
        self.bound_table = bound_table
        self.bound = None if bound_table is None else \
            {"kind": "table", "sha256": hashlib.sha256(bound_table.astype("<u2").tobytes()).hexdigest()}
        self.device = device

    @classmethod
    def from_noise(cls, noise, k, max_error=65535, fg_max_error=None, device=None):
        """The codec whose bound of a voxel is ``k`` noise standard deviations of the voxel's own value under the
        Poisson-Gaussian parameters ``noise`` (what ``estimate_poisson_gaussian`` returns), rounded down, and never
        more than ``max_error`` / ``fg_max_error``: ``bound_table=noise.bound_table(noise, k)``."""
        from aind_exaspim_image_compression.utils.noise import bound_table, pg_params
        codec = cls(max_error, fg_max_error, bound_table=bound_table(noise, k), device=device)
        codec.bound = dict({"kind": "poisson-gaussian"}, **pg_params(noise), k=float(k))
        return codec

    def get_config(self):
        """``"bound"`` describes the table, if there is one: the model and ``k`` it came from, or its SHA-256 (of the
        little-endian bytes).  It documents the store; no decoder needs it."""
        cfg = {"id": self.codec_id, "max_error": self.max_error, "fg_max_error": self.fg_max_error,
               "version": self.version}
        if self.bound is not None:
            cfg["bound"] = dict(self.bound)
        return cfg

    @staticmethod
    def _mask(mask, shape):
        """None, or the mask as a contiguous uint8 array (non-zero = foreground) of the volume's 3-D shape."""
        if mask is None:
            return None
        m = np.asarray(mask)
        if _shape3(m.shape) != tuple(shape):
            raise ValueError(f"mask shape {m.shape} differs from the volume's {tuple(shape)}")
        return np.ascontiguousarray(m != 0, dtype=np.uint8).reshape(-1)

    # -- what a chunk store asks ---------------------------------------------------------------
    def config_entry(self):
        cfg = {"version": self.version, "max_error": self.max_error, "fg_max_error": self.fg_max_error,
               "edge_chunks": "truncated"}
        if self.bound is not None:              # where the bound table came from; no reader needs it
            cfg["bound"] = dict(self.bound)
        return cfg

    @classmethod
    def check_config(cls, cfg):
        if int(cfg["version"]) != cls.version or not 0 <= int(cfg["fg_max_error"]) <= int(cfg["max_error"]) <= 65535:
            raise ValueError("unsupported exac-dctq-block configuration")
        return 2

    @classmethod
    def from_config(cls, cfg):
        return cls(int(cfg["max_error"]), int(cfg["fg_max_error"]))

    # -- what VolumeCodec asks -----------------------------------------------------------------
    def _bound(self, shape, chunk, want_bytes):
        return _native.block_bounded_volume_bound(shape, chunk)

    def _native_encode(self, ctx, d_vol, shape, chunk, operands, **buffers):
        d_mask, d_table = operands
        return ctx.block_bounded_encode(d_vol, shape, chunk, self.max_error, self.fg_max_error, mask=d_mask,
                                        table=d_table, **buffers)

    def _native_decode(self, ctx, d_in, nbytes, d_off, shape, chunk, d_out):
        ctx.block_bounded_decode(d_in, nbytes, d_off, shape, chunk, d_out)

    # -- the calls that take a mask ------------------------------------------------------------
    def encode(self, chunk, mask=None):
        """One uint16 chunk (up to 3-D) -> bytes; its nominal chunk shape is its extent rounded up to multiples
        of 8."""
        return self._encode_chunk(chunk, mask=mask)

    def encode_volume(self, vol, chunk=(64, 64, 64), mask=None, want_bytes=True):
        """Host uint16 array (up to 3-D), optional mask of its shape -> ``EncodedVolume`` (nominal chunk shape,
        typesize 2).  With ``want_bytes=False`` only the sizes are produced (``data`` is None)."""
        return self._encode_volume(vol, chunk, want_bytes, lambda shape: (self._mask(mask, shape), self.bound_table))

    def encode_device(self, ctx, d_vol, shape, chunk=(64, 64, 64), d_mask=None, want_bytes=True, d_table=None):
        """The same for a volume (and a uint8 mask, or None) that already lies in HBM (device pointer holders).
        ``d_table``: this codec's ``bound_table`` on the device (65536 uint16); a codec that has one needs it."""
        if (d_table is None) != (self.bound_table is None):
            raise ValueError("encode_device: d_table goes with a codec that has a bound_table, and only with one")
        return self._encode_device(ctx, d_vol, shape, chunk, want_bytes, (d_mask, d_table))

    def chunk_sizes(self, vol, chunk=(64, 64, 64), mask=None):
        """``len(self.encode(c))`` of every chunk of ``vol`` in one batched device call (what ``compute_cratio``
        takes)."""
        return self.encode_volume(vol, chunk, mask=mask, want_bytes=False).sizes

    def select_steps(self, vol, chunk=(64, 64, 64), mask=None):
        """-> int16 [gz, gy, gx, cz/8, cy/8, cx/8]: the step every block of every chunk takes under this codec's
        bounds (-1: verbatim, -2: outside the volume), whether or not the chunk would then be stored losslessly --
        where the bound binds, block by block."""
        a = np.ascontiguousarray(vol)
        self._check_dtype(a.dtype, "volumes")
        shape, chunk = _shape3(a.shape), tuple(int(c) for c in _shape3(chunk))
        m = self._mask(mask, shape)
        _native.block_bounded_volume_bound(shape, chunk)
        grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
        cb = tuple(c // 8 for c in chunk)
        nb, nbp = int(np.prod(cb)), plane_bytes(chunk)
        ctx = _native.context(self.device)
        d_vol = ctx.to_device(a.reshape(-1))
        d_mask = ctx.to_device(m) if m is not None else None
        d_plane = ctx.alloc(nbp * int(np.prod(grid)))
        d_table = ctx.to_device(self.bound_table) if self.bound_table is not None else None
        try:
            ctx.block_bounded_steps(d_vol, shape, chunk, self.max_error, self.fg_max_error, d_plane, mask=d_mask,
                                    table=d_table)
            plane = d_plane.download((int(np.prod(grid)), nbp), np.uint8)[:, :nb]
        finally:
            d_vol.free()
            d_plane.free()
            if d_mask is not None:
                d_mask.free()
            if d_table is not None:
                d_table.free()
        steps = plane.astype(np.int16)
        steps[plane == STEP_VERBATIM] = -1
        steps[plane == STEP_OUTSIDE] = -2
        return steps.reshape(grid + cb)

    @staticmethod
    def block_steps(enc):
        """Per chunk of an ``EncodedVolume`` the int16 step plane over its nominal block grid (-1: verbatim block,
        -2: block outside the volume), or None for a chunk stored losslessly (mode 0)."""
        if enc.data is None:
            raise ValueError("the EncodedVolume carries sizes only (encode with want_bytes=True)")
        out = []
        for i in range(len(enc.sizes)):
            o = int(enc.offsets[i])
            out.append(parse_header(enc.data[o:o + int(enc.sizes[i])].tobytes())["steps"])
        return out
