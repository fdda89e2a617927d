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
from aind_exaspim_image_compression.utils.chunk_codec import VolumeCodec, _shape3

STEPS = 29
# Q[j] = float32(2^((j - 4) / 4)), j = 0..28: steps 0.5 .. 64
LADDER = np.array([np.float32(2.0 ** ((j - 4) / 4)) for j in range(STEPS)], dtype=np.float32)
HEADER_BYTES = 32
FORMAT_VERSION = 1
MODE_LOSSLESS, MODE_DCT = 0, 1


def pack_dims(extent, chunk):
    """Bytes 12..23 of either bounded format's header: the chunk's extent E, then its nominal shape C (u16 each)."""
    return np.array(list(extent) + list(chunk), dtype="<u2").tobytes()


def parse_dims(raw, who):
    """-> (extent, chunk) from bytes 12..23 of a header; ``ValueError`` (``who``: the format, in the message) unless
    ``C`` is made of multiples of 8 and ``1 <= E <= C``."""
    dims = np.frombuffer(raw[12:24], dtype="<u2").astype(int)
    extent, chunk = tuple(int(v) for v in dims[:3]), tuple(int(v) for v in dims[3:])
    if any(c < 8 or c % 8 for c in chunk):
        raise ValueError(f"{who} chunk stream: chunk axes must be multiples of 8")
    if any(e < 1 or e > c for e, c in zip(extent, chunk)):
        raise ValueError(f"{who} chunk stream: extent outside 1..chunk")
    return extent, chunk


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
    h[12:24] = pack_dims(extent, chunk)
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
    extent, chunk = parse_dims(raw, "bounded")
    return {"mode": int(mode), "j": None if mode == MODE_LOSSLESS else int(j), "q": q, "extent": extent,
            "chunk": chunk}


def _nominal_chunk(extent):
    return tuple(-(-int(e) // 8) * 8 for e in extent)


class BoundedVolumeCodec(VolumeCodec):
    """What the two error-bounded formats add to ``VolumeCodec``: uint16 volumes, streams that keep the nominal chunk
    shape (their index chunks are sized by it) behind a 32-byte header that states it, and a volume bound that is
    also the format's size check.  ``noun`` names the format in messages."""

    typesize = 2
    nominal_chunks = True

    @property
    def _container(self):
        return self.noun, 16, HEADER_BYTES, "16-byte steps "

    def _check_dtype(self, dtype, what):
        if dtype != np.uint16:
            raise ValueError(f"{type(self).__name__} codes uint16 {what}")

    def _check_typesize(self, enc):
        if enc.typesize != 2:
            raise ValueError(f"the {self.noun} codec stores uint16 volumes")

    def _check_volume(self, shape, chunk):
        self._bound(shape, chunk, False)        # raises for sizes the format does not take

    def _stream_geometry(self, raw):
        h = self.parse_header(raw)
        return h["extent"], h["chunk"]

    def _encode_chunk(self, chunk, **operands):
        a = np.ascontiguousarray(chunk)
        self._check_dtype(a.dtype, "chunks")
        if a.size == 0:
            raise ValueError("cannot encode an empty chunk")
        shape = _shape3(a.shape)
        return self.encode_volume(a.reshape(shape), chunk=_nominal_chunk(shape), **operands).chunk_bytes(0)


class BoundedDctCodec(BoundedVolumeCodec):
    """numcodecs-shaped codec of uint16 chunks with a per-voxel error bound, arithmetic on the GPU."""

    codec_id = "exac-dctq"
    version = FORMAT_VERSION
    noun = "bounded"
    parse_header = staticmethod(parse_header)

    def __init__(self, max_error, device=None):
        max_error = int(max_error)
        if not 0 <= max_error <= 65535:
            raise ValueError("max_error must be in [0, 65535]")
        self.max_error = max_error
        self.device = device

    def get_config(self):
        return {"id": self.codec_id, "max_error": self.max_error, "version": self.version}

    # -- what a chunk store asks ---------------------------------------------------------------
    def config_entry(self):
        return {"version": self.version, "max_error": self.max_error, "edge_chunks": "truncated"}

    @classmethod
    def check_config(cls, cfg):
        if int(cfg["version"]) != cls.version or not 0 <= int(cfg["max_error"]) <= 65535:
            raise ValueError("unsupported exac-dctq configuration")
        return 2

    @classmethod
    def from_config(cls, cfg):
        return cls(int(cfg["max_error"]))

    # -- what VolumeCodec asks -----------------------------------------------------------------
    def _bound(self, shape, chunk, want_bytes):
        return _native.bounded_volume_bound(shape, chunk)

    def _native_encode(self, ctx, d_vol, shape, chunk, operands, **buffers):
        return ctx.bounded_encode(d_vol, shape, chunk, self.max_error, **buffers)

    def _native_decode(self, ctx, d_in, nbytes, d_off, shape, chunk, d_out):
        ctx.bounded_decode(d_in, nbytes, d_off, shape, chunk, d_out)

    def encode(self, chunk):
        """One uint16 chunk (up to 3-D) -> bytes; its nominal chunk shape is its extent rounded up to multiples
        of 8."""
        return self._encode_chunk(chunk)

    def ladder_errors(self, vol, chunk=(64, 64, 64)):
        """-> uint32 [gz, gy, gx, 29]: the largest |reconstruction - voxel| of every chunk at every ladder step
        (independent of ``max_error``: the per-chunk rate-distortion picture)."""
        a = np.ascontiguousarray(vol)
        self._check_dtype(a.dtype, "volumes")
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
