"""A local chunk store for the coded volume, in the layout the reference writes its results in.

The reference ends its production path with ``write_zarr(img, output_path, chunks=(1, 1, 64, 64, 64), ...)``
(reference utils/img_util.py:898-950; called from scripts/evaluate_bm4dnet.py): a Zarr v3 array, 5-D
(t, c, z, y, x), one object per 64^3 chunk under ``c/0/0/<z>/<y>/<x>``, each compressed with
Blosc(zstd, shuffle).  Here the chunk streams are EXAC (``utils/chunk_codec.py``), coded on
the MI355X in one batched call, and they go to disk in the same directory layout:

    <path>/zarr.json            array metadata (Zarr v3 keys: shape, data_type, chunk_grid, chunk_key_encoding,
                                fill_value, codecs = [{"name": "exac", "configuration": {...}}])
    <path>/c/0/0/<z>/<y>/<x>    the EXAC stream of chunk (z, y, x): exactly ``codec.encode(chunk)``

With ``codec=BoundedDctCodec(max_error)`` (``utils/bounded_codec.py``) the chunk streams are the
error-bounded lossy ones, and the codec entry reads ``{"name": "exac-dctq", "configuration": {"version": 1,
"max_error": ..., "edge_chunks": "truncated"}}``; with ``codec=BlockBoundedCodec(max_error, fg_max_error)``
(``utils/block_bounded_codec.py``) and an optional ``mask`` they carry a step per 8^3 block, and the
entry reads ``{"name": "exac-dctq-block", "configuration": {"version": 1, "max_error": ..., "fg_max_error": ...,
"edge_chunks": "truncated"}}``, plus ``"bound": {...}`` (the noise model and k, or the table's SHA-256) when the
codec has a bound table.  The readers pick the decoder from ``zarr.json`` and ignore ``"bound"``.

so that a chunk is addressable by its key like any Zarr chunk and ``sum(file sizes)`` is the denominator of
``compute_cratio`` (utils/img_util.py:401-441).  Differences from a stock Zarr array, stated in the metadata:
the codec is this repo's (a generic Zarr reader needs an ``exac`` codec plug-in: ``ExacCodec.decode``), and
edge chunks are stored TRUNCATED to the array (the reference's ``compute_cratio`` slices them that way; an
EXAC stream carries its own chunk shape), not padded to the chunk grid.  Local file system only -- cloud
stores (fsspec / s3 / gs, which ``write_zarr`` accepts) are out of scope.
"""
import json
import os

import numpy as np

from aind_exaspim_image_compression.utils.block_bounded_codec import BlockBoundedCodec
from aind_exaspim_image_compression.utils.bounded_codec import BoundedDctCodec
from aind_exaspim_image_compression.utils.chunk_codec import EncodedVolume, ExacCodec
from aind_exaspim_image_compression.utils.label_codec import LabelCodec
from aind_exaspim_image_compression.utils.store_pyramid import (  # noqa: F401  (re-exported)
    downsample_store, open_multiscale, pyramid_store)
from aind_exaspim_image_compression.utils.store_label_pyramid import (  # noqa: F401  (re-exported)
    downsample_label_store, downsample_label_volume, plan_label_downsample, pyramid_label_store)
from aind_exaspim_image_compression.utils.store_recode import recode_store  # noqa: F401  (re-exported)

FORMAT_NOTE = ("EXAC chunk streams (aind-exaspim-image-compression_amd, DESIGN.md 3.11b); edge chunks truncated to "
               "the array; decode with utils.chunk_codec.ExacCodec.decode or utils.chunk_store.read_zarr")


def _grid(shape3, chunk3):
    return tuple(-(-s // c) for s, c in zip(shape3, chunk3))


def chunk_key(iz, iy, ix):
    """Zarr v3 default chunk key encoding ("/" separator) of chunk (0, 0, iz, iy, ix) of a 5-D array."""
    return os.path.join("c", "0", "0", str(int(iz)), str(int(iy)), str(int(ix)))


# codec id in ``zarr.json`` -> the class that states the entry's configuration, validates one and decodes its streams
CODECS = {cls.codec_id: cls for cls in (ExacCodec, BoundedDctCodec, BlockBoundedCodec, LabelCodec)}


def _data_type(codec, typesize):
    """``data_type`` of a store of ``codec`` (an instance or a class): uint16 / int32 for the image codecs; the label
    codec states its own (uint32 / uint64)."""
    return getattr(codec, "data_types", {2: "uint16", 4: "int32"})[typesize]


def metadata(shape3, chunk3, typesize=2, version=2, attributes=None, codec=None):
    """The ``zarr.json`` document of a stored volume (``codec``: a ``BoundedDctCodec`` or ``BlockBoundedCodec``
    stores its own entry)."""
    codec = codec or ExacCodec(int(typesize), version=int(version))
    name = next(k for k, cls in CODECS.items() if isinstance(codec, cls))     # a subclass stores its parent's format
    return {
        "zarr_format": 3,
        "node_type": "array",
        "shape": [1, 1] + [int(s) for s in shape3],
        "data_type": _data_type(codec, codec.typesize),
        "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": [1, 1] + [int(c) for c in chunk3]}},
        "chunk_key_encoding": {"name": "default", "configuration": {"separator": "/"}},
        "fill_value": 0,
        "codecs": [{"name": name, "configuration": codec.config_entry()}],
        "attributes": dict(attributes or {}, exac_note=FORMAT_NOTE),
        "dimension_names": ["t", "c", "z", "y", "x"],
    }


def write_encoded(enc, output_path, version=2, attributes=None, overwrite=True, codec=None):
    """``EncodedVolume`` (host container: data, offsets, sizes) -> chunk store at ``output_path``.  Host work
    only.  Returns the number of bytes written as chunk streams.  ``codec``: the ``BoundedDctCodec`` or
    ``BlockBoundedCodec`` that made ``enc``, if one did (its entry goes into the metadata)."""
    if enc.data is None:
        raise ValueError("the EncodedVolume carries sizes only (encode with want_bytes=True)")
    gz, gy, gx = _grid(enc.shape, enc.chunk)
    if len(enc.sizes) != gz * gy * gx:
        raise ValueError("EncodedVolume: chunk count does not match its shape and chunk")
    if os.path.exists(os.path.join(output_path, "zarr.json")) and not overwrite:
        raise FileExistsError(output_path)
    os.makedirs(output_path, exist_ok=True)
    total = 0
    k = 0
    for iz in range(gz):
        for iy in range(gy):
            d = os.path.join(output_path, "c", "0", "0", str(iz), str(iy))
            os.makedirs(d, exist_ok=True)
            for ix in range(gx):
                blob = enc.chunk_bytes(k)
                with open(os.path.join(d, str(ix)), "wb") as f:
                    f.write(blob)
                total += len(blob)
                k += 1
    with open(os.path.join(output_path, "zarr.json"), "w") as f:      # last: a store without it is incomplete
        json.dump(metadata(enc.shape, enc.chunk, enc.typesize, version, attributes, codec), f, indent=1)
    return total


def check_metadata(meta):
    """``(shape3, chunk3, typesize, bounded)`` of a ``zarr.json`` document this repository's readers take;
    ``ValueError`` for anything else.  ``bounded``: the chunk streams keep the nominal chunk shape."""
    try:
        if meta["zarr_format"] != 3 or meta["node_type"] != "array":
            raise ValueError("not a Zarr v3 array")
        codecs = meta["codecs"]
        if len(codecs) != 1 or codecs[0]["name"] not in CODECS:
            raise ValueError("the array's codec chain is not [exac], [exac-dctq], [exac-dctq-block] or [exac-labels]")
        cls = CODECS[codecs[0]["name"]]
        typesize = cls.check_config(codecs[0]["configuration"])
        shape5, chunk5 = meta["shape"], meta["chunk_grid"]["configuration"]["chunk_shape"]
        if len(shape5) != 5 or shape5[:2] != [1, 1] or len(chunk5) != 5 or chunk5[:2] != [1, 1]:
            raise ValueError("only (1, 1, z, y, x) arrays with (1, 1, cz, cy, cx) chunks are stored this way")
        if meta["data_type"] != _data_type(cls, typesize):
            raise ValueError("data_type does not match the codec's typesize")
        if meta["chunk_key_encoding"]["name"] != "default" or \
                meta["chunk_key_encoding"]["configuration"].get("separator", "/") != "/":
            raise ValueError("unsupported chunk key encoding")
    except (KeyError, TypeError) as e:
        raise ValueError(f"zarr.json lacks a field this reader needs: {e}") from None
    shape3, chunk3 = tuple(int(s) for s in shape5[2:]), tuple(int(c) for c in chunk5[2:])
    if min(shape3) < 1 or min(chunk3) < 1:
        raise ValueError("empty array or chunk")
    return shape3, chunk3, typesize, cls.nominal_chunks


def pack_streams(blobs):
    """Chunk streams -> ``(data, offsets, sizes)`` of a container: every stream at a multiple of 16 bytes, as the
    device decoders take it."""
    sizes = np.array([len(b) for b in blobs], dtype=np.uint32)
    offsets = np.zeros(len(blobs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum((sizes.astype(np.uint64) + 15) // 16 * 16)
    data = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for b, o in zip(blobs, offsets[:-1]):
        data[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return data, offsets, sizes


def read_encoded(path):
    """Chunk store -> ``(EncodedVolume, metadata)``: the chunk files gathered into one container (every stream
    at a multiple of 16 bytes, as the device decoder takes it).  Host work only; raises ``ValueError`` for
    a store that is not an EXAC array of this layout and ``FileNotFoundError`` for a missing chunk."""
    with open(os.path.join(path, "zarr.json")) as f:
        meta = json.load(f)
    shape3, chunk3, typesize, bounded = check_metadata(meta)
    gz, gy, gx = _grid(shape3, chunk3)
    blobs = []
    for iz in range(gz):
        for iy in range(gy):
            for ix in range(gx):
                with open(os.path.join(path, chunk_key(iz, iy, ix)), "rb") as f:
                    blobs.append(f.read())
    data, offsets, sizes = pack_streams(blobs)
    # the bounded formats keep the nominal chunk shape (their index chunks are sized by it)
    chunk_eff = chunk3 if bounded else tuple(min(c, s) for c, s in zip(chunk3, shape3))
    return EncodedVolume(data, offsets, sizes, shape3, chunk_eff, typesize), meta


def write_zarr(img, output_path, chunks=(1, 1, 64, 64, 64), codec=None, attributes=None, mask=None):
    """The reference's ``write_zarr(img, output_path, chunks=(1, 1, 64, 64, 64))`` with the EXAC chunk coder in
    the place of Blosc (utils/img_util.py:898-950): ``img`` (uint16, promoted to 5-D like the reference; t and
    c must be 1) is coded on the device in one batched call and written as a chunk store.  Returns the
    compression ratio raw bytes / stored chunk bytes -- what ``compute_cratio(img, codec, chunks[2:])`` reports,
    unrounded.  ``mask`` (``BlockBoundedCodec`` only; the shape of ``img`` or of its volume) marks the voxels held to
    the codec's ``fg_max_error``."""
    img = np.asarray(img)
    while img.ndim < 5:
        img = img[np.newaxis, ...]
    if img.ndim != 5 or img.shape[0] != 1 or img.shape[1] != 1:
        raise ValueError("write_zarr stores (1, 1, z, y, x) arrays")
    if len(chunks) != 5 or tuple(chunks[:2]) != (1, 1):
        raise ValueError("chunks must be (1, 1, cz, cy, cx)")
    codec = codec or ExacCodec(2)
    vol = np.ascontiguousarray(img[0, 0])
    if mask is not None and not codec.takes_mask:
        raise ValueError("only a BlockBoundedCodec takes a mask")
    operands = {"mask": mask} if codec.takes_mask else {}
    enc = codec.encode_volume(vol, chunk=tuple(int(c) for c in chunks[2:]), **operands)
    return vol.nbytes / write_encoded(enc, output_path, attributes=attributes, codec=codec)


def read_zarr(path, codec=None):
    """Chunk store -> the (1, 1, z, y, x) array, decoded on the device in one call."""
    enc, meta = read_encoded(path)
    codec = codec or _codec_of(meta)
    return codec.decode_volume(enc)[np.newaxis, np.newaxis]


def read_chunk(path, iz, iy, ix, codec=None):
    """One chunk by its key, decoded alone (random access: what a viewer does)."""
    with open(os.path.join(path, "zarr.json")) as f:
        meta = json.load(f)
    shape3 = meta["shape"][2:]
    chunk3 = meta["chunk_grid"]["configuration"]["chunk_shape"][2:]
    ext = tuple(min(c, s - i * c) for i, c, s in zip((iz, iy, ix), chunk3, shape3))
    if min(ext) < 1:
        raise IndexError("chunk index outside the array")
    with open(os.path.join(path, chunk_key(iz, iy, ix)), "rb") as f:
        blob = f.read()
    codec = codec or _codec_of(meta)
    return codec.decode(blob).reshape(ext)


def open_zarr(path, device=None, max_pool_bytes=1 << 30, mode="r", codec=None):
    """Chunk store -> ``StoredArray`` (``utils/store_read.py``): the (1, 1, z, y, x) array behind
    numpy basic indexing and ``read_patches``, which decode only the chunks a read touches.  Reads ``zarr.json``
    only.  ``max_pool_bytes``: the most decoded chunks a read or a write keeps on the device at a time.
    ``mode="r+"`` opens the array writable (``write_patches`` and item assignment); with the default
    ``"r"`` writes raise.  ``codec``: needed only to write a block-bounded store with a bound table, which the file
    does not hold; a codec whose ``config_entry()`` differs from the stored one raises ``ValueError``."""
    from aind_exaspim_image_compression.utils.store_read import StoredArray
    with open(os.path.join(path, "zarr.json")) as f:
        meta = json.load(f)
    try:
        labels = meta["codecs"][0]["name"] == LabelCodec.codec_id
    except (KeyError, IndexError, TypeError):
        labels = False                              # StoredArray says what is wrong with the document
    if labels:
        from aind_exaspim_image_compression.utils.store_labels import LabelArray
        return LabelArray(path, device=device, max_pool_bytes=max_pool_bytes, mode=mode, codec=codec)
    return StoredArray(path, device=device, max_pool_bytes=max_pool_bytes, mode=mode, codec=codec)


def create_zarr(path, shape, chunks=(1, 1, 64, 64, 64), codec=None, attributes=None, overwrite=False, device=None,
                max_pool_bytes=1 << 30):
    """An empty store -> writable ``StoredArray``: writes ``zarr.json`` only (the document ``write_zarr`` would write
    for an array of ``shape``: (z, y, x) or (1, 1, z, y, x)) and no chunk.  Region writes fill it; a chunk without a
    file counts as zeros for them, while reads of one keep raising.  A store built by aligned writes of a whole
    volume is byte for byte what ``write_zarr`` makes of that volume."""
    shape = tuple(int(s) for s in shape)
    shape = (1,) * (5 - len(shape)) + shape
    if len(shape) != 5 or shape[:2] != (1, 1) or min(shape) < 1:
        raise ValueError("create_zarr stores (1, 1, z, y, x) arrays")
    if len(chunks) != 5 or tuple(chunks[:2]) != (1, 1) or min(int(c) for c in chunks) < 1:
        raise ValueError("chunks must be (1, 1, cz, cy, cx)")
    codec = codec or ExacCodec(2)
    if codec.typesize != 2 and not isinstance(codec, LabelCodec):
        raise NotImplementedError("region writes of int32 (index) stores are not implemented")
    if os.path.exists(os.path.join(path, "zarr.json")) and not overwrite:
        raise FileExistsError(path)
    os.makedirs(path, exist_ok=True)
    chunk3 = codec._chunk(shape[2:], chunks[2:])      # as an EncodedVolume states it: clamped unless nominal
    with open(os.path.join(path, "zarr.json"), "w") as f:
        json.dump(metadata(shape[2:], chunk3, attributes=attributes, codec=codec), f, indent=1)
    return open_zarr(path, device=device, max_pool_bytes=max_pool_bytes, mode="r+", codec=codec)


def _codec_of(meta):
    """The decoder a store's ``zarr.json`` names."""
    entry = meta["codecs"][0]
    return CODECS[entry["name"]].from_config(entry["configuration"])


def _encoder_of(meta):
    """The coder of a store's ``zarr.json``: its decoder, at the stored format version."""
    codec = _codec_of(meta)
    if isinstance(codec, ExacCodec):
        codec = ExacCodec(codec.typesize, version=int(meta["codecs"][0]["configuration"].get("version", 2)))
    return codec
