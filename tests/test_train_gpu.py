"""A BM4DNet training step on NDHWC through the native forward and backward kernels, end to end: gradients
against fp64 CPU autograd of the plain model, with the plain model's own fp32 GPU gradients as the yardstick;
three AdamW steps reproduce bit for bit; the trained weights load as a reference checkpoint."""
import numpy as np
import pytest
import torch

from aind_exaspim_image_compression import inference
from aind_exaspim_image_compression.machine_learning.losses import SignalPreservingLoss
from aind_exaspim_image_compression.machine_learning.train import train_step, trainable_ndhwc
from aind_exaspim_image_compression.machine_learning.unet3d import UNet

pytestmark = pytest.mark.gpu
SHAPES = [(2, 1, 16, 16, 16), (1, 1, 20, 20, 20)]
_ref = {}


def seeded_model():
    torch.manual_seed(1234)
    return UNet()


def batch(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    return x, y, torch.rand(shape, generator=g) < 0.3


def reference_gradients(shape):
    """fp64 CPU autograd of the plain model with the torch loss: computed once per shape, never modified."""
    if shape not in _ref:
        model = seeded_model().double()
        x, y, mask = batch(shape)
        SignalPreservingLoss()(model(x.double()), y.double(), mask).backward()
        _ref[shape] = {n: p.grad.numpy().copy() for n, p in model.named_parameters()}
    return _ref[shape]


def gradient_errors(net, model, shape):
    x, y, mask = (t.cuda() for t in batch(shape))
    model.zero_grad()
    SignalPreservingLoss()(net(x), y, mask).backward()
    out = {}
    for n, p in model.named_parameters():
        g64 = reference_gradients(shape)[n]
        out[n] = float(np.linalg.norm(p.grad.cpu().numpy().astype(np.float64) - g64) / np.linalg.norm(g64))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_against_fp64(shape):
    plain = seeded_model().cuda()
    e_plain = gradient_errors(plain, plain, shape)
    model = seeded_model().cuda()
    twin = trainable_ndhwc(model)
    # the native path runs: a fused module's output carries the new Function
    x = batch(shape)[0].cuda()
    with torch.enable_grad():
        h = twin.inc.double_conv[1](twin.inc.double_conv[0](x))
    assert type(h.grad_fn).__name__ == "_GroupNormLeakyReLUFnBackward"
    e_twin = gradient_errors(twin, model, shape)
    worst = max(e_twin, key=lambda n: e_twin[n] / e_plain[n])
    print(f"{shape}: max rel. gradient error twin {max(e_twin.values()):.3e}, plain {max(e_plain.values()):.3e}; "
          f"worst ratio {e_twin[worst] / e_plain[worst]:.2f} at {worst}")
    for n in e_twin:
        assert e_twin[n] <= 4 * e_plain[n], (n, e_twin[n], e_plain[n])


def three_steps(shape):
    model = seeded_model().cuda()
    twin = trainable_ndhwc(model)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    crit = SignalPreservingLoss()
    x, y, mask = (t.cuda() for t in batch(shape))
    losses = [train_step(twin, opt, crit, x, y, mask) for _ in range(3)]
    return model, twin, torch.stack(losses).cpu().numpy()


def test_three_adamw_steps_and_a_checkpoint(tmp_path):
    """What is compared bit for bit: the FIRST loss -- a forward pass of this repository's kernels, MIOpen's
    forward convolutions and ``torch.cat`` / ``F.pad``, all deterministic.  From the second loss on the weights
    carry MIOpen's backward-weights convolutions, whose solvers may accumulate with atomics (the framework
    documents them as not deterministic), so later losses are compared to rounding only."""
    model, twin, a = three_steps(SHAPES[1])
    _, _, b = three_steps(SHAPES[1])
    print("losses:", a, b)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert a[0].tobytes() == b[0].tobytes()
    np.testing.assert_allclose(a, b, rtol=1e-4)
    # the model -- not the twin -- is the checkpoint: the reference's keys, loadable by load_model
    path = tmp_path / "ckpt.pt"
    torch.save(model.state_dict(), path)
    loaded, transform = inference.load_model(str(path))
    assert list(loaded.state_dict().keys()) == list(UNet().state_dict().keys())
    for k, v in model.state_dict().items():
        assert torch.equal(loaded.state_dict()[k], v)
    patch = np.random.default_rng(0).integers(0, 500, (16, 16, 16)).astype(np.uint16)
    out = inference.predict_patch(patch, loaded, transform)
    assert out.shape == patch.shape and out.dtype == np.uint16
    # a GradScaler that is off is a no-op, one that is on scales the device loss's gradient
    scaler = torch.amp.GradScaler("cuda", enabled=True, init_scale=1024.0)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    x, y, mask = (t.cuda() for t in batch(SHAPES[0]))
    assert torch.isfinite(train_step(twin, opt, SignalPreservingLoss(), x, y, mask, scaler=scaler))
