"""Error-bounded lossy chunk codec: "denoise, then quantise, then entropy-code" as a stored format
(DESIGN.md 3.10b).

Every chunk of a uint16 volume is offered two streams: the 8^3 block-DCT indices of DESIGN.md 3.10 at the
coarsest step of a fixed ladder whose reconstruction stays within ``max_error`` counts of every voxel of the
chunk, coded with EXAC v2 as int32 (mode 1), and the lossless EXAC v2 stream of its voxels (mode 0).  The shorter
one is stored behind a 32-byte header.  Because the reconstruction is an integer result the encoder measures the
exact error every decoder produces, so the bound is a guarantee: every decoded voxel is within ``max_error`` of
the encoder's input, and ``max_error=0`` is lossless.

``BoundedDctCodec`` has the shape of ``utils.chunk_codec.ExacCodec`` (``encode`` / ``decode`` of one chunk, a
batched ``encode_volume`` / ``decode_volume``, ``chunk_sizes`` for ``compute_cratio``); the ladder errors, the
step choice, the quantiser, both entropy coders, the assembly of the container and the decode all run on the
MI355X (``csrc/bounded_kernels.hip``, ``exabm4d_bounded_*``).
"""
import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume, _shape3

STEPS = 29
# Q[j] = float32(2^((j - 4) / 4)), j = 0..28: steps 0.5 .. 64
LADDER = np.array([np.float32(2.0 ** ((j - 4) / 4)) for j in range(STEPS)], dtype=np.float32)
HEADER_BYTES = 32
FORMAT_VERSION = 1
MODE_LOSSLESS, MODE_DCT = 0, 1


def pack_header(mode, j, extent, chunk):
    """The 32-byte header of a chunk stream (mode 0: lossless EXAC uint16 payload, mode 1: EXAC int32 indices at
    step LADDER[j])."""
    h = bytearray(HEADER_BYTES)
    h[0:4] = bytes((ord("E"), ord("Q"), FORMAT_VERSION, int(mode)))
    if mode == MODE_DCT:
        h[4] = int(j)
        h[8:12] = LADDER[int(j)].tobytes()
    else:
        h[4] = 0xFF
    h[12:24] = np.array(list(extent) + list(chunk), dtype="<u2").tobytes()
    return bytes(h)


def parse_header(blob):
    """-> dict(mode, j, q, extent, chunk) of a chunk stream; ``ValueError`` for anything that is not a valid
    header followed by at least one byte of payload."""
    raw = bytes(blob)
    if len(raw) <= HEADER_BYTES:
        raise ValueError("bounded chunk stream: truncated (no payload behind the 32-byte header)")
    if raw[0:2] != b"EQ":
        raise ValueError("bounded chunk stream: bad magic")
    if raw[2] != FORMAT_VERSION:
        raise ValueError(f"bounded chunk stream: unknown format version {raw[2]}")
    mode, j = raw[3], raw[4]
    qbits = raw[8:12]
    if mode == MODE_LOSSLESS:
        if j != 0xFF or qbits != bytes(4):
            raise ValueError("bounded chunk stream: a lossless chunk carries no step")
        q = 0.0
    elif mode == MODE_DCT:
        if j >= STEPS or qbits != LADDER[j].tobytes():
            raise ValueError("bounded chunk stream: the step is not the ladder's Q[j]")
        q = float(LADDER[j])
    else:
        raise ValueError(f"bounded chunk stream: unknown mode {mode}")
    dims = np.frombuffer(raw[12:24], dtype="<u2").astype(int)
    extent, chunk = tuple(int(v) for v in dims[:3]), tuple(int(v) for v in dims[3:])
    if any(c < 8 or c % 8 for c in chunk):
        raise ValueError("bounded chunk stream: chunk axes must be multiples of 8")
    if any(e < 1 or e > c for e, c in zip(extent, chunk)):
        raise ValueError("bounded chunk stream: extent outside 1..chunk")
    return {"mode": int(mode), "j": None if mode == MODE_LOSSLESS else int(j), "q": q, "extent": extent,
            "chunk": chunk}


def _nominal_chunk(extent):
    return tuple(-(-int(e) // 8) * 8 for e in extent)


class BoundedDctCodec:
    """numcodecs-shaped codec of uint16 chunks with a per-voxel error bound, arithmetic on the GPU."""

    codec_id = "exac-dctq"
    version = FORMAT_VERSION

    def __init__(self, max_error, device=None):
        max_error = int(max_error)
        if not 0 <= max_error <= 65535:
            raise ValueError("max_error must be in [0, 65535]")
        self.max_error = max_error
        self.device = device

    def get_config(self):
        return {"id": self.codec_id, "max_error": self.max_error, "version": self.version}

    # -- one chunk ---------------------------------------------------------------------------
    def encode(self, chunk):
        """One uint16 chunk (up to 3-D) -> bytes; its nominal chunk shape is its extent rounded up to multiples
        of 8."""
        a = np.ascontiguousarray(chunk)
        if a.dtype != np.uint16:
            raise ValueError("BoundedDctCodec codes uint16 chunks")
        if a.size == 0:
            raise ValueError("cannot encode an empty chunk")
        shape = _shape3(a.shape)
        return self.encode_volume(a.reshape(shape), chunk=_nominal_chunk(shape)).chunk_bytes(0)

    def decode(self, buf, out=None):
        """bytes of one chunk -> 1-D uint16 array (or filled ``out``).  The header is validated on the host."""
        raw = bytes(buf)
        h = parse_header(raw)
        pad = (-len(raw)) % 16
        data = np.frombuffer(raw + bytes(pad), dtype=np.uint8)
        enc = EncodedVolume(data, np.array([0, data.size], dtype=np.uint64), np.array([len(raw)], dtype=np.uint32),
                            h["extent"], h["chunk"], 2)
        res = self.decode_volume(enc).reshape(-1)
        if out is not None:
            np.copyto(np.asarray(out).reshape(-1), res)
            return out
        return res

    # -- a whole volume ------------------------------------------------------------------------
    def encode_volume(self, vol, chunk=(64, 64, 64), want_bytes=True):
        """Host uint16 array (up to 3-D) -> ``EncodedVolume`` (nominal chunk shape, typesize 2).  With
        ``want_bytes=False`` only the sizes are produced (``data`` is None)."""
        a = np.ascontiguousarray(vol)
        if a.dtype != np.uint16:
            raise ValueError("BoundedDctCodec codes uint16 volumes")
        shape = _shape3(a.shape)
        ctx = _native.context(self.device)
        d_vol = ctx.to_device(a.reshape(-1))
        try:
            return self.encode_device(ctx, d_vol, shape, chunk, want_bytes)
        finally:
            d_vol.free()

    def encode_device(self, ctx, d_vol, shape, chunk=(64, 64, 64), want_bytes=True):
        """The same for a volume that already lies in HBM (``d_vol``: device pointer holder)."""
        shape, chunk = _shape3(shape), tuple(int(c) for c in _shape3(chunk))
        cap = _native.bounded_volume_bound(shape, chunk)
        nchunks = int(np.prod([-(-s // c) for s, c in zip(shape, chunk)]))
        d_sizes = ctx.alloc(4 * nchunks)
        d_off = ctx.alloc(8 * (nchunks + 1))
        d_out = ctx.alloc(cap) if want_bytes else None
        try:
            _, container = ctx.bounded_encode(d_vol, shape, chunk, self.max_error, out=d_out,
                                              out_capacity=cap if want_bytes else 0, offsets=d_off, sizes=d_sizes)
            sizes = d_sizes.download((nchunks,), np.uint32)
            offsets = d_off.download((nchunks + 1,), np.uint64)
            data = d_out.download((container,), np.uint8) if want_bytes else None
        finally:
            d_sizes.free()
            d_off.free()
            if d_out is not None:
                d_out.free()
        return EncodedVolume(data, offsets, sizes, shape, chunk, 2)

    @staticmethod
    def _checked(enc):
        """(data, offsets, shape, chunk) of a container that passed the host checks."""
        if enc.typesize != 2:
            raise ValueError("the bounded codec stores uint16 volumes")
        shape, chunk = _shape3(enc.shape), _shape3(enc.chunk)
        offsets = np.ascontiguousarray(enc.offsets, dtype=np.uint64)
        data = np.ascontiguousarray(enc.data, dtype=np.uint8)
        nchunks = int(np.prod([-(-s // c) for s, c in zip(shape, chunk)]))
        if offsets.size != nchunks + 1 or np.any(np.diff(offsets.astype(np.int64)) < HEADER_BYTES) or \
                int(offsets[-1]) > data.size or np.any(offsets % 16):
            raise ValueError("malformed bounded container: offsets are not ascending 16-byte steps inside the data")
        _native.bounded_volume_bound(shape, chunk)          # raises for sizes the format does not take
        return data, offsets, shape, chunk

    def decode_volume(self, enc):
        """``EncodedVolume`` of this format -> host uint16 array of ``enc.shape``."""
        shape = self._checked(enc)[2]
        ctx = _native.context(self.device)
        d_vol = ctx.alloc(2 * int(np.prod(shape)))
        try:
            self.decode_device(ctx, enc, d_vol)
            return d_vol.download(shape, np.uint16)
        finally:
            d_vol.free()

    def decode_device(self, ctx, enc, d_out):
        """``decode_volume`` without the download: ``EncodedVolume`` -> ``d_out`` (device pointer holder or address,
        ``prod(enc.shape)`` uint16), decoded when the call returns."""
        data, offsets, shape, chunk = self._checked(enc)
        d_in = ctx.to_device(data if data.size else np.zeros(16, np.uint8))
        d_off = ctx.to_device(offsets)
        try:
            ctx.bounded_decode(d_in, data.size, d_off, shape, chunk, d_out)
        finally:
            d_in.free()
            d_off.free()

    def chunk_sizes(self, vol, chunk=(64, 64, 64)):
        """``len(self.encode(c))`` of every chunk of ``vol`` in one batched device call (what ``compute_cratio``
        takes)."""
        return self.encode_volume(vol, chunk, want_bytes=False).sizes

    def ladder_errors(self, vol, chunk=(64, 64, 64)):
        """-> uint32 [gz, gy, gx, 29]: the largest |reconstruction - voxel| of every chunk at every ladder step
        (independent of ``max_error``: the per-chunk rate-distortion picture)."""
        a = np.ascontiguousarray(vol)
        if a.dtype != np.uint16:
            raise ValueError("BoundedDctCodec codes uint16 volumes")
        shape, chunk = _shape3(a.shape), tuple(int(c) for c in _shape3(chunk))
        _native.bounded_volume_bound(shape, chunk)
        grid = tuple(-(-s // c) for s, c in zip(shape, chunk))
        ctx = _native.context(self.device)
        d_vol = ctx.to_device(a.reshape(-1))
        d_err = ctx.alloc(4 * STEPS * int(np.prod(grid)))
        try:
            ctx.dctq_ladder_errors(d_vol, shape, chunk, d_err)
            return d_err.download(grid + (STEPS,), np.uint32)
        finally:
            d_vol.free()
            d_err.free()

    @staticmethod
    def chunk_steps(enc):
        """float32 [nchunks]: the step q of every chunk of an ``EncodedVolume`` (0 for a lossless chunk)."""
        if enc.data is None:
            raise ValueError("the EncodedVolume carries sizes only (encode with want_bytes=True)")
        out = np.zeros(len(enc.sizes), dtype=np.float32)
        for i in range(len(enc.sizes)):
            o = int(enc.offsets[i])
            out[i] = parse_header(enc.data[o:o + int(enc.sizes[i])].tobytes())["q"]
        return out
