"""``SignalPreservingLoss`` on the device (csrc/nn_grad_kernels.hip) against the fp64 restatement: the value to
4 * 2^-24 * L (each element is evaluated in fp64 and the partials are fp64, so one rounding remains), the
gradient elementwise to 4 * 2^-24 * |ref|."""
import numpy as np
import pytest
import torch

import nn_grad_pyref as ref
from aind_exaspim_image_compression.machine_learning.losses import SignalPreservingLoss

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MASKS = {"fp32": torch.float32, "uint8": torch.uint8, "bool": torch.bool}
_inputs = {}


def inputs(n):
    """(pred, target, mask) as fp32 / fp32 / 0-1 numpy arrays; element 0 has d = 0 (where n > 1)."""
    if n not in _inputs:
        rng = np.random.default_rng(n)
        pred = rng.standard_normal(n).astype(np.float32)
        target = (pred + rng.standard_normal(n).astype(np.float32) * rng.choice([1e-4, 1e-2, 1.0], n)).astype(np.float32)
        if n > 1:
            target[0] = pred[0]
        _inputs[n] = (pred, target, (rng.random(n) < 0.3).astype(np.float32))
    return _inputs[n]


@pytest.mark.parametrize("fg_weight", [0.0, 20.0])
@pytest.mark.parametrize("mask_kind", sorted(MASKS))
@pytest.mark.parametrize("n", [1, 4097, 2 * 64 ** 3])
def test_value_and_gradient(n, mask_kind, fg_weight):
    pred, target, mask = inputs(n)
    shape = (2, 1, 64, 64, 64) if n == 2 * 64 ** 3 else (n,)
    p = torch.from_numpy(pred).cuda().view(shape).requires_grad_(True)
    t = torch.from_numpy(target).cuda().view(shape)
    m = torch.from_numpy(mask).cuda().view(shape).to(MASKS[mask_kind])
    crit = SignalPreservingLoss(fg_weight=fg_weight)
    loss = crit(p, t, m)
    assert type(loss.grad_fn).__name__ == "_CharbonnierLossFnBackward"
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    want = ref.charbonnier_loss(pred, target, mask, fg_weight)
    err = abs(float(loss.detach()) - want)
    print(f"loss n={n} {mask_kind} w={fg_weight}: |L - ref| / L = {err / want / U:.3f} u")
    assert err <= 4 * U * want
    (g1,) = torch.autograd.grad(loss, p, retain_graph=True)
    want_g = ref.charbonnier_loss_backward(pred, target, mask, fg_weight)
    got = g1.cpu().numpy().reshape(-1).astype(np.float64)
    assert np.all(np.abs(got - want_g) <= 4 * U * np.abs(want_g))
    if n > 1:
        assert got[0] == 0.0                                   # d = 0
    # grad_output 1024: exact scaling, bit for bit
    (g2,) = torch.autograd.grad(loss, p, grad_outputs=torch.tensor(1024.0, device="cuda"))
    assert torch.equal(g2, g1 * 1024.0)
    # the torch expression agrees (the path every other input takes)
    plain = ((1.0 + fg_weight * m) * torch.sqrt((p - t) * (p - t) + 1e-6)).mean()
    assert abs(float(plain.detach()) - want) <= 1e-5 * want


def test_nan_prediction_gives_a_nan_loss():
    pred, target, mask = (torch.from_numpy(a).cuda() for a in inputs(4097))
    pred = pred.clone()
    pred[1234] = float("nan")
    assert torch.isnan(SignalPreservingLoss()(pred, target, mask))


def test_ndhwc_storage_order_and_fallbacks():
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (2, 8, 3, 4, 5)
    p = torch.randn(shape, generator=g, device="cuda").to(memory_format=torch.channels_last_3d).requires_grad_(True)
    t = torch.randn(shape, generator=g, device="cuda").to(memory_format=torch.channels_last_3d)
    m = (torch.rand(shape, generator=g, device="cuda") < 0.3).to(memory_format=torch.channels_last_3d)
    crit = SignalPreservingLoss()
    loss = crit(p, t, m)
    assert type(loss.grad_fn).__name__ == "_CharbonnierLossFnBackward"
    loss.backward()
    want = ref.charbonnier_loss(p.detach().cpu().numpy(), t.cpu().numpy(), m.cpu().numpy())
    assert abs(float(loss.detach()) - want) <= 4 * U * want
    want_g = ref.charbonnier_loss_backward(p.detach().cpu().numpy(), t.cpu().numpy(), m.cpu().numpy())
    assert p.grad.stride() == p.stride()
    assert np.all(np.abs(p.grad.cpu().numpy() - want_g) <= 4 * U * np.abs(want_g))
    # a mask in another layout, a broadcasting mask, fp64: the torch expression
    for args in ((p, t, m.contiguous()), (p, t, m[:, :1]), (p.double(), t.double(), m)):
        out = crit(*args)
        assert type(out.grad_fn).__name__ != "_CharbonnierLossFnBackward"
        assert abs(float(out.detach()) - want) <= 1e-5 * want or args[2].shape != p.shape
