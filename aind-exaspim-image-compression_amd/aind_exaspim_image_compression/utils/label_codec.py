"""Lossless chunk codec for segmentation labels: ``exac-labels``.

The reference keeps its label volume behind ``tensorstore`` as a neuroglancer-precomputed uint64 array
(``TrainDataset._load_segmentation``, reference ``machine_learning/data_handling.py:176-214``) and reads 64^3 label
patches out of it.  ``LabelCodec`` is the chunk codec of such a volume in this package's chunk store: unsigned 32- or
64-bit ids, each chunk cut into 8^3 blocks, each block a sorted palette of its distinct ids plus packed indices of 0,
1, 2, 4 or 8 bits (or the raw values past 256 ids).  The idea is that of neuroglancer's ``compressed_segmentation``; the
layout is this repository's own and is not that wire format.  A stream is a pure function of the chunk's values --
there is one valid encoding -- so the bytes of the GPU coder, of the numpy restatement in ``tests/label_pyref.py`` and
of repeated runs are identical.

``validate_stream`` is the host check every reader runs on a stream before its bytes go to the device.
"""
import numpy as np

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.utils.chunk_codec import VolumeCodec, _nchunks, _shape3

MAGIC = b"EXLB"
HEADER = 32
DTYPES = {4: np.dtype(np.uint32), 8: np.dtype(np.uint64)}
_ENTRY = np.dtype([("at", "<u4"), ("k", "<u2"), ("bits", "u1"), ("zero", "u1")])
_BITS_OF_K = np.full(257, -1, dtype=np.int64)       # index bits of a palette of k entries
for _most, _bits in ((256, 8), (16, 4), (4, 2), (2, 1), (1, 0)):
    _BITS_OF_K[1:_most + 1] = _bits


def validate_stream(raw, typesize, extent=None):
    """The extent (ez, ey, ex) of one well-formed ``exac-labels`` stream of ``typesize``; ``ValueError`` for anything
    else: magic, version, typesize, the extent (against ``extent``, where the reader knows it), the block count, the
    total, and every table entry -- k agreeing with bits, payloads contiguous in block order and inside the stream.
    Header and table only: the payloads are not looked at (the kernels clamp every index they read)."""
    raw = bytes(raw)
    if len(raw) < HEADER or raw[:4] != MAGIC:
        raise ValueError("not an exac-labels stream")
    head = np.frombuffer(raw, dtype="<u2", count=2, offset=4)
    words = np.frombuffer(raw, dtype="<u4", count=6, offset=8)
    if int(head[0]) != 1:
        raise ValueError("exac-labels stream of an unknown version")
    if int(head[1]) != int(typesize):
        raise ValueError("exac-labels stream of another typesize")
    ext = tuple(int(v) for v in words[:3])
    nblocks, total = int(words[3]), int(words[4])
    if min(ext) < 1 or ext[0] * ext[1] * ext[2] > 1 << 27 or (extent is not None and ext != tuple(extent)):
        raise ValueError("exac-labels stream of another extent than its chunk's")
    if nblocks != int(np.prod([-(-e // 8) for e in ext])) or int(words[5]) != 0:
        raise ValueError("exac-labels stream with an inconsistent block count")
    if total != len(raw) or total % 8 or total < HEADER + 8 * nblocks:
        raise ValueError("exac-labels stream whose total is not its length (truncated?)")
    table = np.frombuffer(raw, dtype=_ENTRY, count=nblocks, offset=HEADER)
    at, k, bits = (table[f].astype(np.int64) for f in ("at", "k", "bits"))
    is_raw = bits == 8 * typesize
    if np.any(table["zero"]) or np.any(is_raw & (k != 0)) or np.any(~is_raw & (k > 256)) or \
            np.any(~is_raw & (bits != _BITS_OF_K[np.minimum(k, 256)])):
        raise ValueError("exac-labels stream with a block whose k disagrees with its bits")
    size = np.where(is_raw, 512 * typesize, (k * typesize + 7) // 8 * 8 + 64 * bits)
    if np.any(8 * at + size > total):
        raise ValueError("exac-labels stream with a table offset past its end")
    begin = np.concatenate(([(HEADER + 8 * nblocks) // 8], (at + size // 8)[:-1]))
    if np.any(at != begin) or 8 * int(at[-1]) + int(size[-1]) != total:
        raise ValueError("exac-labels stream whose payloads are not ascending and contiguous in block order")
    return ext


class LabelCodec(VolumeCodec):
    """numcodecs-shaped lossless codec of uint32 (``typesize=4``) or uint64 (``typesize=8``) label chunks, coded and
    decoded on the GPU."""

    codec_id = "exac-labels"
    nominal_chunks = False
    takes_mask = False
    data_types = {4: "uint32", 8: "uint64"}         # ``data_type`` of a store of this codec (utils/chunk_store.py)
    _container = ("exac-labels", 16, HEADER + 16, "at multiples of 16 bytes ")

    def __init__(self, typesize=8, device=None):
        if typesize not in DTYPES:
            raise ValueError("typesize must be 4 (uint32) or 8 (uint64)")
        self.typesize = int(typesize)
        self.device = device

    @property
    def dtype(self):
        return DTYPES[self.typesize]

    def _element_dtype(self):
        return self.dtype

    def get_config(self):
        return {"id": self.codec_id, "typesize": self.typesize, "version": 1}

    # -- what a chunk store asks ---------------------------------------------------------------
    def config_entry(self):
        return {"version": 1, "typesize": self.typesize, "edge_chunks": "truncated"}

    @classmethod
    def check_config(cls, cfg):
        if int(cfg["version"]) != 1 or int(cfg["typesize"]) not in DTYPES or cfg.get("edge_chunks") != "truncated":
            raise ValueError("unsupported exac-labels configuration")
        return int(cfg["typesize"])

    @classmethod
    def from_config(cls, cfg):
        return cls(cls.check_config(cfg))

    # -- what VolumeCodec asks -----------------------------------------------------------------
    def _check_dtype(self, dtype, what):
        if np.dtype(dtype) != self.dtype:
            raise ValueError(f"LabelCodec(typesize={self.typesize}) codes {self.dtype} {what}, not {np.dtype(dtype)}")

    def _check_typesize(self, enc):
        if enc.typesize != self.typesize:
            raise ValueError("EncodedVolume of another typesize")

    def _bound(self, shape, chunk, want_bytes):
        bound = _native.label_encode_bound(self.typesize, shape, chunk)      # also the geometry's check
        return bound if want_bytes else 0

    @staticmethod
    def _check_volume(shape, chunk):
        n = int(np.prod(shape))
        if n < 1 or n > (1 << 40):
            raise ValueError("malformed exac-labels container: implausible volume shape")

    def _checked(self, enc):
        """The scaffold's container checks, then every stream's header and table against its chunk's extent: nothing
        is uploaded before all of them passed."""
        data, offsets, shape, chunk = super()._checked(enc)
        sizes = np.ascontiguousarray(enc.sizes, dtype=np.int64).reshape(-1)
        if sizes.size != _nchunks(shape, chunk):
            raise ValueError("malformed exac-labels container: one size per chunk")
        grid = [-(-s // c) for s, c in zip(shape, chunk)]
        i = 0
        for iz in range(grid[0]):
            for iy in range(grid[1]):
                for ix in range(grid[2]):
                    ext = tuple(min(c, s - j * c) for j, c, s in zip((iz, iy, ix), chunk, shape))
                    o = int(offsets[i])
                    if o + int(sizes[i]) > int(offsets[i + 1]):
                        raise ValueError("malformed exac-labels container: a stream overlaps the next")
                    validate_stream(data[o:o + int(sizes[i])].tobytes(), self.typesize, ext)
                    i += 1
        return data, offsets, shape, chunk

    def _native_encode(self, ctx, d_vol, shape, chunk, operands, **buffers):
        return ctx.label_encode(d_vol, self.typesize, shape, chunk, **buffers)

    def _native_decode(self, ctx, d_in, nbytes, d_off, shape, chunk, d_out):
        ctx.label_decode(d_in, nbytes, d_off, self.typesize, shape, chunk, d_out)

    def _stream_geometry(self, raw):
        ext = validate_stream(raw, self.typesize)
        return ext, ext

    # -- one chunk ---------------------------------------------------------------------------
    def encode(self, buf):
        """One (up to 3-D) chunk -> bytes."""
        a = np.ascontiguousarray(buf)
        self._check_dtype(a.dtype, "chunks")
        if a.size == 0:
            raise ValueError("cannot encode an empty chunk")
        shape = _shape3(a.shape)
        return self.encode_volume(a.reshape(shape), chunk=shape).chunk_bytes(0)
