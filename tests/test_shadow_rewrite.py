"""``predict``'s NDHWC shadow (``inference._ndhwc_shadow`` / ``_fuse_norm_act``) on the models of ``nn_zoo``, on
the CPU: the rewrite decides what each zoo entry declares (which GroupNorm + LeakyReLU pairs it fuses, which of
them run in place, which convolution biases move into the kernels, which resamplings go native), it leaves the
caller's model alone, and -- every module falls back to the framework here -- the shadow computes what the model
computes, to fp32 summation order.  The same models against fp64 on the GPU: ``test_shadow_zoo_gpu.py``."""
import numpy as np
import pytest
import torch

import nn_zoo as Z

from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning import unet3d


def decisions(shadow):
    """What the rewrite did, counted per slot of the module tree (the fields of ``nn_zoo.Entry``)."""
    mods = [m for _, m in shadow.named_modules(remove_duplicate=False)]
    fused = [m for m in mods if isinstance(m, inference.FusedGroupNormLeakyReLU)]
    wrapped = [m for m in mods if isinstance(m, inference._ResampleNDHWC)]
    return {"pairs": len(fused), "inplace": sum(bool(m.inplace) for m in fused),
            "biases": sum(m.conv_bias is not None for m in fused), "gn": sum(m.native_channels for m in fused),
            "pool": sum(m.kind == "pool" for m in wrapped), "up": sum(m.kind == "up" for m in wrapped)}


def declared(entry):
    return {k: getattr(entry, k) for k in ("pairs", "inplace", "biases", "gn", "pool", "up")}


@pytest.mark.parametrize("name", sorted(Z.ZOO))
def test_rewrite_decisions(name):
    entry = Z.ZOO[name]
    for half in (False, True):
        shadow = inference._ndhwc_shadow(entry.build(), half=half)
        assert decisions(shadow) == declared(entry), name
        mods = list(shadow.modules())
        assert not any(m.training for m in mods)
        # a pair that writes in place sits right behind a Conv3d of its container; a resampling is wrapped once
        for m in mods:
            if isinstance(m, torch.nn.Sequential):
                for i, f in enumerate(m):
                    if isinstance(f, inference.FusedGroupNormLeakyReLU):
                        assert f.inplace == (i > 0 and isinstance(m[i - 1], torch.nn.Conv3d))
                        assert f.half == half
            if isinstance(m, inference._ResampleNDHWC):
                assert isinstance(m.inner, (torch.nn.MaxPool3d, torch.nn.Upsample))
    # a bias moved into a fused pair is gone from its convolution; every other convolution keeps its own
    model = entry.build()
    shadow = inference._ndhwc_shadow(model)
    had = sum(m.bias is not None for _, m in model.named_modules(remove_duplicate=False)
              if isinstance(m, torch.nn.Conv3d))
    kept = sum(m.bias is not None for _, m in shadow.named_modules(remove_duplicate=False)
               if isinstance(m, torch.nn.Conv3d))
    assert had - kept == entry.biases


@pytest.mark.parametrize("name", sorted(Z.ZOO))
def test_shadow_leaves_the_model_alone(name):
    """The caller's model after its shadows were built (fused and not, fp32 and half): the same modules, a
    bit-identical ``state_dict``, every Conv3d with the bias it had, every parameter in its memory format."""
    model = Z.ZOO[name].build()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    types = [type(m) for _, m in model.named_modules(remove_duplicate=False)]
    biases = [m.bias is not None for m in model.modules() if isinstance(m, torch.nn.Conv3d)]
    formats = [p.is_contiguous() for p in model.parameters()]
    for fuse in (True, False):
        for half in (False, True):
            inference._ndhwc_shadow(model, fuse=fuse, half=half)
    after = model.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k].dtype == v.dtype and torch.equal(after[k].view(torch.int32), v.view(torch.int32)), k
    assert [type(m) for _, m in model.named_modules(remove_duplicate=False)] == types
    assert [m.bias is not None for m in model.modules() if isinstance(m, torch.nn.Conv3d)] == biases
    assert [p.is_contiguous() for p in model.parameters()] == formats
    assert not model.training


@pytest.mark.parametrize("name", sorted(Z.ZOO))
def test_shadow_matches_the_model_on_cpu(name):
    """On the CPU every module of the shadow takes the framework's path: the shadow's output is the model's up to
    fp32 summation order (a bias added after the convolution instead of inside it, NDHWC convolutions), and its
    input is left as it was."""
    entry = Z.ZOO[name]
    model = entry.build()
    x = Z.make_input(entry)
    shadow = inference._ndhwc_shadow(model)
    xs = x.contiguous(memory_format=torch.channels_last_3d)
    x0 = xs.clone()
    with torch.no_grad():
        want = model(x).double()
        got = shadow(xs).double()
    assert torch.equal(xs.view(torch.int32), x0.view(torch.int32))
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    scale = float(want.abs().max())
    assert err <= 1e-5 * max(1.0, scale), f"{name}: shadow differs from the model by {err:.3g} (max |y| {scale:.3g})"


@pytest.mark.parametrize("net,native", [("UNet", 18), ("N2V2UNet", 17)])
def test_unet_pairs_stay_fused_and_in_place(net, native):
    """The production path keeps its shape: every one of the U-Net's 18 GroupNorm + LeakyReLU pairs is fused
    behind its convolution, runs in place and carries that convolution's bias; in N2V2UNet 17 of its 18 are
    channel counts the kernels take (GroupNorm(8, 16) falls back at run time)."""
    torch.manual_seed(0)
    for half in (False, True):
        d = decisions(inference._ndhwc_shadow(getattr(unet3d, net)().eval(), half=half))
        assert d["pairs"] == 18 and d["inplace"] == 18 and d["biases"] == 18 and d["gn"] == native, d
        assert (d["pool"], d["up"]) == ((4, 4) if net == "UNet" else (0, 4)), d
