"""``predict``'s NDHWC shadow on the models of ``nn_zoo`` (beyond this package's U-Nets) on the GPU, in fp32, fp16
and bf16, against the fp64 forward of the same model on the CPU -- run the way ``predict`` runs it: built with
``_ndhwc_shadow(model, half=...)``, the half types under ``torch.autocast``, gradients off.

Per entry and precision:
  * bound -- the rule of ``test_nn_kernels_gpu.test_shadow_forward_against_fp64``: the fused shadow's largest
    error is at most twice that of the unfused shadow (``fuse=False``: the framework's modules) in the same
    precision, plus a floor (see ``floor``);
  * the input, and every tensor the model reads again after a fused call (``Entry.keep``), is bit-identical
    after the forward: a pair that wrote in place into a live tensor fails here whatever its numbers;
  * the native entries ran as often as the entry declares (a silent fallback fails too).
End to end: ``predict`` with ``fast=True`` against ``fast=False`` on two of the models."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

import nn_zoo as Z
from test_inference_gpu import TF_CFG
from test_nn_half_gpu import _count_native
from test_oracle_golden import tiling_volume

from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning import transforms as T

pytestmark = pytest.mark.gpu
PRECISIONS = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}
# unit round-off of the storage type
UNIT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def floor(prec, want):
    """The bound's additive floor.  fp32: 1e-5 of the output's range, as for the U-Net.  fp16 / bf16: 4 u of the
    output's range, u the storage type's unit round-off (2^-11, 2^-8).  Where the framework's GroupNorm runs in
    fp32 under autocast and hands an fp32 result on, the fused kernels round theirs once to the storage type
    (u |y|), and a following sum of two half tensors rounds once more (u |out|); each of |y|, |out| is taken
    as at most twice the output's range."""
    ptp = float(np.ptp(want))
    return 1e-5 * ptp if prec == "fp32" else 4 * UNIT[prec] * ptp


@functools.lru_cache(maxsize=None)
def fp64_forward(name):
    entry = Z.ZOO[name]
    model = entry.build()
    with torch.no_grad():
        return copy.deepcopy(model).double()(Z.make_input(entry).double()).numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(_BITS[a.dtype]), b.view(_BITS[b.dtype]))


def shadow_forward(shadow, x, prec, keep=()):
    """One forward of ``shadow`` as ``predict`` runs it; returns (fp64 numpy output, native calls per entry,
    {name: (the output of module ``name`` as the model saw it, a copy taken then)})."""
    kept = {}
    mods = dict(shadow.named_modules())
    hooks = [mods[k].register_forward_hook(lambda m, i, o, k=k: kept.__setitem__(k, (o, o.clone()))) for k in keep]
    amp = PRECISIONS[prec]
    try:
        with torch.no_grad(), (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
            seen, out = _count_native(lambda: shadow(x))
    finally:
        for h in hooks:
            h.remove()
    return out.double().cpu().numpy(), seen, kept


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", sorted(Z.ZOO))
def test_zoo_shadow_against_fp64(name, prec):
    entry = Z.ZOO[name]
    want = fp64_forward(name)
    model = entry.build().cuda()
    half = PRECISIONS[prec] is not None
    x = Z.make_input(entry).cuda().contiguous(memory_format=torch.channels_last_3d)
    x0 = x.clone()
    plain, _, _ = shadow_forward(inference._ndhwc_shadow(model, fuse=False, half=half), x, prec)
    assert same_bits(x, x0)
    got, seen, kept = shadow_forward(inference._ndhwc_shadow(model, half=half), x, prec, entry.keep)
    e_fused = float(np.max(np.abs(got - want)))
    e_plain = float(np.max(np.abs(plain - want)))
    bound = 2 * e_plain + floor(prec, want)
    print(f"{name} {prec}: fused {e_fused:.3g}, unfused {e_plain:.3g}, {e_fused / bound:.3g} x the bound")
    assert e_fused <= bound, f"{name} {prec}: fused shadow {e_fused:.3g} = {e_fused / bound:.3g} x the bound " \
                             f"(unfused {e_plain:.3g})"
    assert same_bits(x, x0), f"{name} {prec}: the forward changed its input"
    assert sorted(kept) == sorted(entry.keep)
    for k, (live, copy_then) in kept.items():
        assert same_bits(live, copy_then), f"{name} {prec}: the output of {k!r} changed after it was produced"
    counts = {k: len(v) for k, v in seen.items()}
    assert counts == {"gn": entry.gn, "pool": entry.pool, "up": entry.up}, f"{name} {prec}: native calls {counts}"


@pytest.mark.parametrize("name", ["preact_residual", "shared_conv_1_16"])
def test_predict_fast_against_fast_off(name):
    """``predict`` fp32, default fast path (the shadow, the fused kernels) against ``fast=False`` (the model as
    given) on a 40 x 56 x 72 volume: 12 patches of 32^3 in batches of 5, so a short tail batch of 2.  The
    criterion of ``test_ndhwc_shadow_matches_the_reference_cpu_output_and_leaves_the_model_alone``."""
    entry = Z.ZOO[name]
    model = entry.build().cuda()
    tf = T.build_transform(TF_CFG)
    vol = tiling_volume((40, 56, 72), seed=8)
    kw = dict(batch_size=5, patch_size=32, overlap=8, trim=3, verbose=False)
    seen, a = _count_native(lambda: inference.predict(vol, model, tf, **kw))
    b = inference.predict(vol, model, tf, fast=False, **kw)
    assert len(seen["gn"]) == 3 * entry.gn                # three batches, every fused pair native
    assert a.shape == b.shape == vol.shape and a.dtype == b.dtype == np.uint16
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    print(f"{name}: fast vs fast=False: max |delta| {d.max()}, share > 1: {np.mean(d > 1):.3g}")
    assert np.mean(d > 1) < 1e-3
