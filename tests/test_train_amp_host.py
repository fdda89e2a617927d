"""The host side of training under fp16 / bf16 autocast: argument checks and how ``trainable_ndhwc(model,
precision=...)`` builds its twin.  No GPU: on CPU tensors every rewritten module is the framework's fallback."""
import pytest
import torch

from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning.losses import SignalPreservingLoss
from aind_exaspim_image_compression.machine_learning.train import train_step, trainable_ndhwc
from aind_exaspim_image_compression.machine_learning.unet3d import UNet

REWRITTEN = (inference.FusedGroupNormLeakyReLU, inference._ResampleNDHWC)


def seeded_model():
    torch.manual_seed(1234)
    return UNet()


def test_unknown_precision_is_a_value_error_before_any_work():
    def boom(*a, **k):
        raise AssertionError("the network ran")
    with pytest.raises(ValueError, match="precision"):
        train_step(boom, None, boom, None, None, None, precision="fp8")
    with pytest.raises(ValueError, match="precision"):
        trainable_ndhwc(seeded_model(), precision="fp8")


def test_half_twin_shares_parameters_and_flags_its_modules():
    model = seeded_model()
    twin = trainable_ndhwc(model, precision="bf16")
    for a, b in zip(model.parameters(), twin.parameters()):
        assert a is b and a.dtype == torch.float32
    mods = [m for m in twin.modules() if isinstance(m, REWRITTEN)]
    assert sum(isinstance(m, inference.FusedGroupNormLeakyReLU) for m in mods) == 18
    assert sum(isinstance(m, inference._ResampleNDHWC) for m in mods) == 8
    assert all(m.half and m.trainable for m in mods)
    assert list(model.state_dict().keys()) == list(UNet().state_dict().keys())


def test_default_twin_is_built_without_half():
    twin = trainable_ndhwc(seeded_model())
    mods = [m for m in twin.modules() if isinstance(m, REWRITTEN)]
    assert len(mods) == 26 and all(m.trainable and not m.half for m in mods)
    assert all(not m.half for m in trainable_ndhwc(seeded_model(), precision="fp32").modules()
               if isinstance(m, REWRITTEN))


def test_half_twin_on_cpu_is_the_plain_model():
    """Forward and backward of the twin on CPU tensors are the framework's modules on the shared Parameters: the
    plain model's output and every parameter gradient, bit for bit."""
    model = seeded_model()
    twin = trainable_ndhwc(model, precision="bf16")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1, 16, 16, 16, generator=g)
    y = x + 0.1 * torch.randn(x.shape, generator=g)
    mask = torch.rand(x.shape, generator=g) < 0.3
    crit = SignalPreservingLoss()
    out = model(x)
    crit(out, y, mask).backward()
    want = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()
    got = twin(x)
    crit(got, y, mask).backward()
    assert torch.equal(got, out)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, want[n]), n
