"""Plain numpy restatement of ``predict``'s overlap tiling (reference inference.py:69-116, :153-199), the yardstick
of ``exabm4d_tile_gather_u16_dev``, ``exabm4d_tile_stitch_u16_dev`` and ``inference.predict_store``.

TEST INFRASTRUCTURE ONLY.  Every step is one explicit fp32 operation, as in tests/stream_pyref.py, so the GPU tests
compare with ``assert_array_equal``.  tests/test_store_predict_host.py checks ``gather_patches`` and ``stitch``
without a GPU against what the reference's own ``predict`` fed a recording model and returned
(tests/golden/stitch.npz, made by tests/golden/make_stitch_golden.py).
"""
import itertools

import numpy as np

import stream_pyref
from oracle.host_oracle import TransformOracle

F32 = np.float32


def patch_starts(shape, patch, overlap):
    """Patch corners ``range(0, dim - patch + stride, stride)`` per axis, z outermost (inference.py:202-252)."""
    stride = patch - overlap
    return list(itertools.product(*(range(0, int(n) - patch + stride, stride) for n in shape)))


def random_predictions(n, patch, seed):
    """Seeded fp32 network outputs (n, patch, patch, patch): mostly in and around [0, 1], negative values and -0.0.
    tests/golden/make_stitch_golden.py feeds them to the reference's ``predict``; the tests regenerate them."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.3, 1.3, (n, patch, patch, patch)).astype(F32)
    p[rng.random(p.shape) < 0.05] = F32(-0.0)
    return p


def gather_patches(counts, cfg, patch, starts):
    """(N, patch, patch, patch) fp32 inputs of the network: the transformed image (inference.py:69) cut at
    ``starts`` and padded with ZEROS at the high end of each axis (``add_padding``: the pad is 0.0 in the transformed
    domain, not ``forward(0)``)."""
    counts = np.asarray(counts)
    assert counts.dtype == np.uint16 and counts.ndim == 3
    img = TransformOracle(cfg).forward(counts)
    out = np.zeros((len(starts), patch, patch, patch), dtype=F32)
    for n, (z, y, x) in enumerate(starts):
        sub = img[z:z + patch, y:y + patch, x:x + patch]
        out[n, :sub.shape[0], :sub.shape[1], :sub.shape[2]] = sub
    return out


def stitch(preds, starts, shape, trim, cfg):
    """uint16 counts of a volume of ``shape`` from the network's outputs ``preds`` (N, patch, patch, patch) at
    ``starts``: the trimmed cores added one patch after the other into fp32 accumulators that start at +0.0
    (inference.py:81-103), then ``stream_pyref.tile_finalize`` (inference.py:113-116)."""
    preds = np.asarray(preds)
    assert preds.dtype == F32 and preds.ndim == 4 and len(preds) == len(starts)
    patch = preds.shape[1] if len(preds) else 0
    core = patch - 2 * trim
    acc = np.zeros(shape, dtype=F32)
    wgt = np.zeros(shape, dtype=F32)
    for pred, start in zip(preds, starts):
        s = [c + trim for c in start]
        e = [max(min(a + core, d), a) for a, d in zip(s, shape)]
        box = tuple(slice(a, b) for a, b in zip(s, e))
        part = pred[tuple(slice(trim, trim + b - a) for a, b in zip(s, e))]
        acc[box] = acc[box] + part
        wgt[box] = wgt[box] + F32(1.0)
    return stream_pyref.tile_finalize(cfg, acc, wgt)
