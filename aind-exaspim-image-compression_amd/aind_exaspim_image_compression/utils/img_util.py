"""Compression-ratio operators (SURVEY.md section 8 "next" row f-1).

``compute_cratio`` keeps the reference's signature and semantics (reference
``utils/img_util.py:401-441``): C-order chunks of ``patch_shape``, ``codec.encode(chunk)``,
ratio rounded to two decimals.  The codec is whatever object the caller passes -- the reference
passes ``numcodecs.blosc.Blosc(cname="zstd", clevel=5|6, shuffle=SHUFFLE)`` (``evaluate.py:40``,
``scripts/evaluate_bm4dnet.py:140``), which is third-party and not part of this repo.

``utils.chunk_codec.ExacCodec`` is a codec object of that shape whose arithmetic runs on the
MI355X (EXAC v2: predictive, context-modelled rANS; ``version=1`` / ``ShuffleRansCodec``: byte
shuffle + order-0 rANS per byte plane); given it, ``compute_cratio`` codes all chunks in one
batched device call.

``shuffled_entropy_cratio`` is the MI355X-side rate floor of that codec: a HIP kernel builds, per 64^3 chunk,
the histograms of the two byte planes Blosc's SHUFFLE filter produces; the zeroth-order entropy
of those planes bounds what an order-0 entropy coder behind the shuffle can reach.  It is a proxy
for rate-distortion sweeps that keeps the volume in HBM, NOT the Blosc/zstd byte count (zstd also
exploits repeats); parity of the histograms with numpy is exact and tested.
"""
import numpy as np

from aind_exaspim_image_compression import _native


def compute_cratio(img, codec, patch_shape=(64, 64, 64)):
    """Chunked compression ratio = total raw bytes / total ``codec.encode`` bytes."""
    img = np.asarray(img)
    if img.ndim == 5:
        img = img[0, 0]
    img = np.ascontiguousarray(img, dtype=np.uint16)
    if img.ndim == 3 and hasattr(codec, "chunk_sizes"):
        # a device codec (utils/chunk_codec.ExacCodec): all chunks in one batched call;
        # the sizes are exactly len(codec.encode(chunk)) of the loop below
        return round(img.nbytes / int(codec.chunk_sizes(img, patch_shape).sum(dtype=np.uint64)), 2)
    raw = 0
    packed = 0
    grids = [range(0, s, c) for s, c in zip(img.shape, patch_shape)]
    for z0 in grids[0]:
        for y0 in grids[1]:
            for x0 in (grids[2] if len(grids) > 2 else [0]):
                chunk = np.ascontiguousarray(img[z0:z0 + patch_shape[0], y0:y0 + patch_shape[1],
                                                 x0:x0 + patch_shape[2]])
                packed += len(codec.encode(chunk))
                raw += chunk.nbytes
    return round(raw / packed, 2)


def compress_and_decompress(img, codec, patch_shape=(64, 64, 64)):
    """-> ``(decoded, cratio)``: the image after a round trip through ``codec`` chunk by chunk, and the chunked
    compression ratio rounded like ``compute_cratio`` (the counterpart of the reference's
    ``compress_and_decompress_jpeg``, ``utils/img_util.py:474-514``).  ``decoded`` has the input's shape; 5-D
    input is accepted like ``compute_cratio``.  A device codec (``ExacCodec``, ``BoundedDctCodec``) takes one
    batched encode and one batched decode."""
    img = np.asarray(img)
    vol = img[0, 0] if img.ndim == 5 else img
    vol = np.ascontiguousarray(vol, dtype=np.uint16)
    if vol.ndim == 3 and hasattr(codec, "encode_volume") and hasattr(codec, "decode_volume"):
        enc = codec.encode_volume(vol, patch_shape)
        decoded = codec.decode_volume(enc).reshape(vol.shape)
        packed = enc.nbytes
    else:
        decoded = np.empty_like(vol)
        packed = 0
        grids = [range(0, s, c) for s, c in zip(vol.shape, patch_shape)]
        for z0 in grids[0]:
            for y0 in grids[1]:
                for x0 in (grids[2] if len(grids) > 2 else [0]):
                    sl = (slice(z0, z0 + patch_shape[0]), slice(y0, y0 + patch_shape[1]),
                          slice(x0, x0 + patch_shape[2]))[:vol.ndim]
                    chunk = np.ascontiguousarray(vol[sl])
                    blob = codec.encode(chunk)
                    packed += len(blob)
                    decoded[sl] = np.asarray(codec.decode(blob)).reshape(chunk.shape)
    out = decoded.reshape(img.shape) if img.ndim == 5 else decoded
    return out, round(vol.nbytes / packed, 2)


def chunk_byte_histograms(img, patch_shape=(64, 64, 64), device=None):
    """[nchunks, 2, 256] uint32 histograms of the low / high byte planes of every chunk (GPU)."""
    vol = np.ascontiguousarray(img, dtype=np.uint16)
    if vol.ndim != 3:
        raise ValueError("expected a 3-D uint16 volume")
    ctx = _native.context(device)
    n = int(np.prod([-(-s // c) for s, c in zip(vol.shape, patch_shape)]))
    d_vol = ctx.to_device(vol)
    d_hist = ctx.alloc(n * 512 * 4)
    try:
        ctx.chunk_byte_histograms(d_vol, vol.shape, patch_shape, d_hist)
        ctx.sync()
        return d_hist.download((n, 2, 256), np.uint32)
    finally:
        d_vol.free()
        d_hist.free()


def entropy_bytes(hist):
    """Zeroth-order entropy bound in bytes of the byte planes described by ``hist[..., 256]``."""
    h = np.asarray(hist, dtype=np.float64)
    n = h.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        bits = -np.where(h > 0, h * np.log2(h / n), 0.0).sum(axis=-1)
    return bits / 8.0


def shuffled_entropy_cratio(img, patch_shape=(64, 64, 64), device=None):
    """Raw bytes / order-0 entropy bound of the byte-shuffled chunks, rounded like compute_cratio."""
    hist = chunk_byte_histograms(img, patch_shape, device)
    raw = float(hist[:, 0, :].sum()) * 2.0
    return round(raw / max(float(entropy_bytes(hist).sum()), 1.0), 2)


# ---- quality metrics on device ----------------------------------------
def _device_pair(img1, img2):
    """Upload two images with one common element type: uint16 when both are, float64 otherwise
    (the reference widens everything to float64: img_util.py:981-982)."""
    a, b = np.asarray(img1), np.asarray(img2)
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions")
    if not (a.dtype == np.uint16 and b.dtype == np.uint16):
        a, b = a.astype(np.float64), b.astype(np.float64)
    ctx = _native.context()
    return ctx, a, ctx.to_device(np.ascontiguousarray(a).reshape(-1)), \
        ctx.to_device(np.ascontiguousarray(b).reshape(-1))


def ssim3D(img1, img2, data_range=None, window_size=16):
    """Structural similarity of two 3-D images with a cubic uniform window (reference
    ``utils/img_util.py:953-1003``): local moments by ``scipy.ndimage.uniform_filter`` semantics
    ("reflect" boundary), ``C1 = (0.01 L)^2``, ``C2 = (0.03 L)^2``, mean of
    ``num / (max(den, 1e-8) + 1e-6)``.

    The moments and the SSIM map are formed by one fp64 HIP kernel that marches running box sums
    along z (``exabm4d_ssim3d_dev``); for uint16 input and the default power-of-two window the
    local moments are exact, and the result differs from the reference only by the summation order
    of the final mean (relative 1e-15)."""
    ctx, a, d_a, d_b = _device_pair(img1, img2)
    try:
        if a.ndim != 3:
            raise ValueError("ssim3D expects 3-D images")
        n = int(a.size)
        if data_range is None:
            lo1, hi1 = ctx.minmax(d_a, a.dtype, n)
            lo2, hi2 = ctx.minmax(d_b, a.dtype, n)
            data_range = max(hi1 - lo1, hi2 - lo2)
        c1 = (0.01 * data_range) ** 2
        c2 = (0.03 * data_range) ** 2
        total = ctx.ssim3d_sum(d_a, d_b, a.dtype, a.shape, window_size, c1, c2)
        return np.float64(total) / n
    finally:
        d_a.free()
        d_b.free()


def _abs_error_stats(img1, img2):
    ctx, a, d_a, d_b = _device_pair(img1, img2)
    try:
        n = int(a.size)
        return ctx.masked_error_stats(d_a, a.dtype, d_b, a.dtype, None, n), n
    finally:
        d_a.free()
        d_b.free()


def compute_mae(img1, img2):
    """Mean absolute error (reference ``utils/img_util.py`` compute_mae)."""
    out, n = _abs_error_stats(img1, img2)
    return float(out[1] / n)


def compute_lmax(img1, img2):
    """Maximum absolute error (reference ``utils/img_util.py`` compute_lmax)."""
    out, _ = _abs_error_stats(img1, img2)
    return float(out[6])


def mip_to_uint8(mip, low_pct=1.0, high_pct=99.9):
    """A projection plane stretched to 8 bits for viewing: the arithmetic of the reference's ``save_mip_png``
    (``machine_learning/train.py:464-488``) without the file.  The plane is taken as float32; its ``low_pct``-th
    percentile maps to 0 and its ``high_pct``-th to 255 (when the upper one does not exceed the lower one it is the
    lower one plus 1), values between them linearly, rounded half to even, and everything outside is clipped.
    Writing the image stays with the caller."""
    plane = np.asarray(mip).astype(np.float32)
    black, white = np.percentile(plane, (low_pct, high_pct))
    if white <= black:
        white = black + 1.0
    stretched = np.clip((plane - black) / (white - black), 0.0, 1.0)
    return np.rint(stretched * 255).astype(np.uint8)


# -- patch coordinates (reference ``utils/img_util.py`` get_patch / get_start_end / get_slices / is_inbounds) ------
def _half_extent(shape):
    """The three half edge lengths, rounded down: what the reference's patch arithmetic is made of."""
    half = np.asarray(shape)[:3] // 2
    return [int(h) for h in half]


def get_start_end(voxel, shape, is_center=True):
    """(start, end) of the patch ``get_patch`` reads: per axis ``voxel - half`` .. ``voxel + half`` with ``half`` the
    edge length halved and rounded down.  With ``is_center=False`` the start is ``voxel`` as it was passed, and --
    the reference's quirk, kept -- the end is still ``voxel + half``."""
    half = _half_extent(shape)
    corner = voxel if not is_center else [voxel[a] - half[a] for a in (0, 1, 2)]
    return corner, [voxel[a] + half[a] for a in (0, 1, 2)]


def get_patch(img, voxel, shape, is_center=True):
    """The patch of a 5-D (t, c, z, y, x) image at ``voxel``: ``img[0, 0, z0:z1, y0:y1, x0:x1]`` of
    ``get_start_end``, so ``img`` may be an array or a ``chunk_store.open_zarr`` array.  Where the reference gives up
    -- no start coordinate is non-negative, or no end coordinate lies below the image's extent -- it returns
    ``np.ones(shape)``, and so does this."""
    if len(img.shape) != 5:
        raise AssertionError("get_patch reads (t, c, z, y, x) images, not %d-D ones" % len(img.shape))
    lo, hi = get_start_end(voxel, shape, is_center=is_center)
    extent = img.shape[2:]
    some_start_inside = max(lo) >= 0
    some_end_inside = min(h - n for h, n in zip(hi, extent)) < 0
    if not (some_start_inside and some_end_inside):
        return np.ones(shape)
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    return img[(0, 0) + box]


def get_slices(center, shape):
    """One slice per axis of the patch of ``shape`` around ``center``: it begins half an edge (rounded down) below
    the centre and is exactly ``shape`` long."""
    half = _half_extent(shape)
    return tuple(slice(c - h, c - h + n) for c, h, n in zip(center, half, shape))


def is_inbounds(voxel, shape):
    """Whether ``voxel`` lies inside a grid of ``shape``."""
    (z, y, x), (nz, ny, nx) = voxel, shape
    return bool(0 <= z < nz and 0 <= y < ny and 0 <= x < nx)
