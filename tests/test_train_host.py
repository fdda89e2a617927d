"""The training layer's host side: ``trainable_ndhwc`` shares the model's Parameters, ``SignalPreservingLoss``
restates the reference's, and the NDHWC modules' default (``trainable=False``) behaves as before (CPU)."""
import copy

import numpy as np
import torch

from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning.losses import SignalPreservingLoss, charbonnier
from aind_exaspim_image_compression.machine_learning.train import train_step, trainable_ndhwc
from aind_exaspim_image_compression.machine_learning.unet3d import UNet


def small_batch(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 1, 16, 16, 16), generator=g, dtype=dtype)
    y = torch.randn((1, 1, 16, 16, 16), generator=g, dtype=dtype)
    return x, y, torch.rand((1, 1, 16, 16, 16), generator=g) < 0.3


def test_trainable_ndhwc_shares_the_models_parameters():
    torch.manual_seed(0)
    model = UNet()
    keys = list(model.state_dict().keys())
    ids = {id(p) for p in model.parameters()}
    twin = trainable_ndhwc(model)
    assert {id(p) for p in twin.parameters()} == ids == {id(p) for p in model.parameters()}
    assert {id(b) for b in twin.buffers()} == {id(b) for b in model.buffers()}
    assert list(model.state_dict().keys()) == keys
    assert any(isinstance(m, inference.FusedGroupNormLeakyReLU) and m.trainable and not m.inplace
               and m.conv_bias is None for m in twin.modules())
    assert all(m.bias is not None for m in twin.modules() if isinstance(m, torch.nn.Conv3d))
    # one SGD step on the MODEL's parameters changes the twin's output
    x, y, mask = small_batch(torch.float32)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with torch.no_grad():
        before = twin(x).clone()
    loss = train_step(twin, opt, SignalPreservingLoss(), x, y, mask)
    assert loss.dim() == 0 and not loss.requires_grad and np.isfinite(float(loss))
    with torch.no_grad():
        after = twin(x)
        assert not torch.equal(before, after)
        assert torch.equal(after, model(x))            # both run the framework's modules on the CPU


def test_twin_gradients_equal_the_plain_models_in_fp64():
    torch.manual_seed(1)
    model = UNet().double()
    plain = copy.deepcopy(model)
    twin = trainable_ndhwc(model)
    x, y, mask = small_batch(torch.float64, 1)
    crit = SignalPreservingLoss()
    crit(twin(x), y, mask).backward()
    crit(plain(x), y, mask).backward()
    for (name, p), q in zip(model.named_parameters(), plain.parameters()):
        np.testing.assert_allclose(p.grad.numpy(), q.grad.numpy(), rtol=1e-10,
                                   atol=1e-10 * float(q.grad.abs().max()), err_msg=name)


def test_charbonnier_approximates_l1():
    c = charbonnier(torch.tensor([3.0, -4.0]), eps=1e-3)
    assert torch.allclose(c, torch.tensor([3.0, 4.0]), atol=1e-2)


def test_loss_defaults_and_attributes():
    loss = SignalPreservingLoss()
    assert (loss.fg_weight, loss.eps) == (20.0, 1e-3)
    assert isinstance(SignalPreservingLoss(5, 1).fg_weight, float)


def test_fg_weight_zero_is_the_plain_charbonnier_mean():
    g = torch.Generator().manual_seed(2)
    pred, target = torch.randn((2, 1, 4, 4, 4), generator=g), torch.randn((2, 1, 4, 4, 4), generator=g)
    fg = torch.ones(2, 1, 4, 4, 4)
    got = SignalPreservingLoss(fg_weight=0.0)(pred, target, fg)
    assert torch.equal(got, charbonnier(pred - target, 1e-3).mean())
    # the reference's case: zeros against ones
    assert abs(float(SignalPreservingLoss(fg_weight=0.0)(torch.zeros(2, 1, 4, 4, 4), fg, fg)) - 1.0) < 5e-3


def test_foreground_error_is_weighted_more():
    loss = SignalPreservingLoss(fg_weight=10.0)
    target = torch.zeros(1, 1, 2, 2, 2)
    fg = torch.zeros(1, 1, 2, 2, 2)
    fg[0, 0, 0, 0, 0] = 1.0
    pred_fg = torch.zeros(1, 1, 2, 2, 2)
    pred_fg[0, 0, 0, 0, 0] = 1.0
    pred_bg = torch.zeros(1, 1, 2, 2, 2)
    pred_bg[0, 0, 1, 1, 1] = 1.0
    lf, lb = float(loss(pred_fg, target, fg)), float(loss(pred_bg, target, fg))
    assert lf > lb
    # (11 * 1 + 7 * eps) / 8 against (1 + 10 * eps + 7 * eps) / 8
    assert abs(lf - (11 * np.sqrt(1 + 1e-6) + 7e-3) / 8) < 1e-6 and abs(lb - (np.sqrt(1 + 1e-6) + 17e-3) / 8) < 1e-6


def test_gradient_moves_the_prediction_toward_the_target():
    loss = SignalPreservingLoss(fg_weight=5.0)
    pred = torch.zeros(1, 1, 2, 2, 2, requires_grad=True)
    loss(pred, torch.ones(1, 1, 2, 2, 2), torch.ones(1, 1, 2, 2, 2)).backward()
    assert pred.grad is not None and torch.all(pred.grad < 0)
    assert torch.allclose(pred.grad, torch.full_like(pred.grad, -6.0 / 8), atol=1e-5)


def test_broadcasting_masks_take_the_torch_expression():
    pred, target = torch.zeros(2, 1, 2, 2, 2), torch.ones(2, 1, 2, 2, 2)
    got = SignalPreservingLoss(fg_weight=1.0)(pred, target, torch.ones(1, 1, 1, 1, 2))
    assert abs(float(got) - 2.0) < 1e-2


def test_default_modules_keep_the_frameworks_autograd():
    """``trainable=False`` under ``enable_grad``: the framework's modules run, as before this flag existed."""
    norm, act = torch.nn.GroupNorm(8, 32), torch.nn.LeakyReLU(0.01)
    fused = inference.FusedGroupNormLeakyReLU(norm, act)
    assert fused.trainable is False
    x = torch.randn(1, 32, 4, 4, 4).to(memory_format=torch.channels_last_3d)
    with torch.enable_grad():
        y = fused(x)
        assert "LeakyRelu" in type(y.grad_fn).__name__
        assert torch.equal(y, act(norm(x)))
        for inner, tag in ((torch.nn.MaxPool3d(2), "MaxPool"), (torch.nn.Upsample(
                scale_factor=2, mode="trilinear", align_corners=True), "Upsample")):
            m = inference._ResampleNDHWC(inner)
            assert m.trainable is False
            out = m(x.clone().requires_grad_(True))
            assert tag in type(out.grad_fn).__name__
    # the trainable flag changes nothing off the device either
    with torch.enable_grad():
        y = inference.FusedGroupNormLeakyReLU(norm, act, inplace=False, trainable=True)(x)
        assert "LeakyRelu" in type(y.grad_fn).__name__
