"""Shared helpers for the tests: deterministic synthetic data (numpy only), a directory for sockets."""
import contextlib
import os
import pathlib
import shutil
import tempfile

import numpy as np


def synth_volume(shape, seed=0, sigma=24.0, pedestal=37.0, as_u16=False):
    """Pedestal + a few blurred bright 'neurites' + N(0, sigma) noise."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    clean = np.full(shape, pedestal, dtype=np.float64)
    for _ in range(max(2, int(np.prod(shape)) // 40000)):
        p0 = rng.uniform(0, 1, 3) * np.array(shape)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        amp = np.exp(rng.uniform(np.log(100), np.log(3000)))
        # distance of every voxel to the line p0 + t d
        v = np.stack([zz - p0[0], yy - p0[1], xx - p0[2]], axis=-1)
        t = v @ d
        dist2 = np.sum(v * v, axis=-1) - t * t
        clean += amp * np.exp(-dist2 / (2 * 1.5 ** 2))
    noisy = clean + rng.normal(0, sigma, shape)
    if as_u16:
        return np.rint(np.clip(noisy, 0, 65535)).astype(np.uint16), clean
    return noisy.astype(np.float32), clean


def psnr(a, b, peak):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(peak ** 2 / mse)


def metric_inputs(seed, shape=(40, 36, 44)):
    """(pred_u16, pred_f32, raw_u16, target_f32, fg) of one synthetic example."""
    rng = np.random.default_rng(seed)
    clean = np.full(shape, 120.0)
    clean[10:20, 8:30, 12:18] = 2500.0
    clean[25:27, :, 20:22] = 9000.0
    raw = np.rint(np.clip(clean + rng.normal(0, 24, shape), 0, 65535)).astype(np.uint16)
    raw[:2] = 0                                           # zero padding outside the imaged volume
    target = np.clip(clean + rng.normal(0, 3, shape), 0, 65535).astype(np.float32)
    pred_f32 = np.clip(clean + rng.normal(0, 5, shape), 0, 65535).astype(np.float32)
    pred_f32[30, 30, 30] = 7000.0                         # a hallucinated bright background voxel
    pred_u16 = np.rint(pred_f32).astype(np.uint16)
    fg = clean > 1000
    return pred_u16, pred_f32, raw, target, fg


class GuardedView:
    """`n` elements of `dtype` at element offset `k` inside a larger DeviceBuffer, with a guard band of
    `guard` bytes (a multiple of 16, so k = 0 is 16-byte aligned) on both sides; every byte that is not
    data holds `fill`.  ``ptr`` is what a kernel is handed; ``check_output`` / ``check_untouched`` download
    the WHOLE buffer, so a store outside [0, n) of the view shows wherever it lands."""

    def __init__(self, ctx, dtype, n, k=0, data=None, guard=256, fill=0xA5):
        self.dtype, self.n = np.dtype(dtype), int(n)
        assert guard % 16 == 0
        self.lo = guard + int(k) * self.dtype.itemsize
        self.hi = self.lo + self.n * self.dtype.itemsize
        self.host = np.full(self.hi + self.dtype.itemsize * 8 + guard, fill, dtype=np.uint8)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1)
            assert data.size == self.n
            self.host[self.lo:self.hi] = data.view(np.uint8)
        self.buf = ctx.to_device(self.host)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + self.lo

    def _download(self):
        return self.buf.download(self.host.shape, np.uint8)

    def check_output(self, want, what="", upto=None):
        """The view equals `want` exactly and every byte around it is as uploaded.  With `upto`, `want` holds
        only the view's first `upto` elements: those are compared, the rest of the view is left unspecified,
        and the bytes around the view are checked all the same."""
        got = self._download()
        want = np.ascontiguousarray(want, dtype=self.dtype).reshape(-1)
        n = self.n if upto is None else int(upto)
        assert want.size == n <= self.n
        np.testing.assert_array_equal(got[self.lo:self.lo + n * self.dtype.itemsize].view(self.dtype), want,
                                      err_msg=f"{what}: values")
        np.testing.assert_array_equal(got[:self.lo], self.host[:self.lo], err_msg=f"{what}: bytes before the view")
        np.testing.assert_array_equal(got[self.hi:], self.host[self.hi:], err_msg=f"{what}: bytes after the view")

    def check_untouched(self, what=""):
        np.testing.assert_array_equal(self._download(), self.host, err_msg=f"{what}: an input was written")

    def free(self):
        self.buf.free()


def match_tables(ctx, vols, sigma, c_match, u16=True):
    """Block matching's tables of a volume (3-D: `(gz, gy, gx, 16)`) or of a batch of volumes (4-D:
    `(batch, gz, gy, gx, 16)`), through `blockmatch_u16` (`u16`: biased uint16 counts) or `blockmatch` (fp32):
    upload, launch, sync, download; both device buffers are freed whatever happens."""
    from aind_exaspim_image_compression import _native
    shape = vols.shape[-3:]
    batch = vols.shape[0] if vols.ndim == 4 else 1
    g = [len(_native.grid_positions(n)) for n in shape]
    d_vol = ctx.to_device(np.ascontiguousarray(vols))
    d_keys = ctx.alloc(batch * g[0] * g[1] * g[2] * 16 * 4)
    try:
        (ctx.blockmatch_u16 if u16 else ctx.blockmatch)(d_vol, shape, sigma, c_match, d_keys, batch=batch)
        ctx.sync()
        return d_keys.download((batch, *g, 16) if vols.ndim == 4 else (*g, 16), np.uint32)
    finally:
        d_vol.free()
        d_keys.free()


# The library's defaults of the options the tests change (exabm4d_set_option).
OPTION_DEFAULTS = {
    "bm_carry": 1, "bm_xcd_mode": 2, "force_generic_bm": 0, "bm_guarded_copy": 0, "bm_int": 1,
    "zero_overlap": 1, "host_pipeline": 1, "stage_chunks": 0, "stage_strip": 3, "stage_pairvol": 1,
}


@contextlib.contextmanager
def ctx_options(ctx, **values):
    """Sets the context's options `values`; on exit every option set is back at the library's default.  Yields a
    function that sets further options under the same promise (a test that goes through several settings)."""
    touched = []

    def set_options(**more):
        for name, value in more.items():
            assert name in OPTION_DEFAULTS, f"{name}: name its default in OPTION_DEFAULTS"
            if name not in touched:
                touched.append(name)
            ctx.set_option(name, value)

    try:
        set_options(**values)
        yield set_options
    finally:
        for name in touched:
            ctx.set_option(name, OPTION_DEFAULTS[name])


@contextlib.contextmanager
def socket_dir(tmp_path, room=0):
    """A directory for the broker's AF_UNIX socket (plus `room` bytes of sub-directories): tmp_path when the
    socket path fits in the 107 bytes such a path may hold, else a fresh short directory under /tmp -- pytest's
    tmp_path under a long TMPDIR or user name goes past the limit."""
    from aind_exaspim_image_compression import broker
    if len(str(tmp_path)) + room + 1 + len(os.path.basename(broker.socket_path(0))) <= 107:
        yield pathlib.Path(tmp_path)
        return
    d = tempfile.mkdtemp(prefix="exb-", dir="/tmp")
    try:
        yield pathlib.Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)
