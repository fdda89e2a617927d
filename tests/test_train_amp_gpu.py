"""A BM4DNet training step under fp16 / bf16 autocast on the NDHWC kernels, end to end: every norm pair, max-pool
and up-sampling native in both directions on the half-width tensors; gradients against fp64 CPU autograd of the plain
model, with the plain model under the framework's own autocast as the yardstick; ``train_step`` with and without a
``GradScaler``; an overflowing step is seen by the scaler and skipped."""
import numpy as np
import pytest
import torch

from test_nn_half_gpu import DTYPES
from test_train_gpu import SHAPES, batch, reference_gradients, seeded_model

from aind_exaspim_image_compression import _native, inference
from aind_exaspim_image_compression.machine_learning.losses import SignalPreservingLoss
from aind_exaspim_image_compression.machine_learning.train import train_step, trainable_ndhwc
from aind_exaspim_image_compression.machine_learning.unet3d import UNet

pytestmark = pytest.mark.gpu
ENTRIES = {"gn_fwd": "groupnorm_lrelu_ndhwc_train", "pool_fwd": "maxpool2_ndhwc", "up_fwd": "upsample2_trilinear_ndhwc",
           "gn_bwd": "groupnorm_lrelu_bwd_ndhwc", "pool_bwd": "maxpool2_bwd_ndhwc",
           "up_bwd": "upsample2_trilinear_bwd_ndhwc", "gn_infer": "groupnorm_lrelu_ndhwc"}
LOSS_SCALE = 2.0 ** 10


def count_native(fn):
    """Run fn() and return the dtype codes the native NDHWC entries were called with, per entry."""
    seen = {k: [] for k in ENTRIES}
    C = _native.Context
    real = {k: getattr(C, name) for k, name in ENTRIES.items()}

    def spy(kind):
        def f(self, *a, **k):
            seen[kind].append(k.get("dtype", _native.DTYPE_F32))
            return real[kind](self, *a, **k)
        return f
    for k, name in ENTRIES.items():
        setattr(C, name, spy(k))
    try:
        out = fn()
    finally:
        for k, name in ENTRIES.items():
            setattr(C, name, real[k])
    return seen, out


def forward_backward(net, shape, dtype):
    x, y, mask = (t.cuda() for t in batch(shape))
    with torch.autocast("cuda", dtype=dtype):
        loss = SignalPreservingLoss()(net(x), y, mask)
    (loss * LOSS_SCALE).backward()
    return loss


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_layer_runs_native_in_half_both_directions(name, shape):
    dtype = DTYPES[name]
    code = inference._NATIVE_DTYPES[dtype]
    model = seeded_model().cuda()
    twin = trainable_ndhwc(model, precision=name)
    convs = []
    orig_conv = torch.nn.Conv3d.forward

    def conv_spy(self, x):
        convs.append((x.dtype, x.shape[1] == 1 or x.is_contiguous(memory_format=torch.channels_last_3d)))
        return orig_conv(self, x)
    torch.nn.Conv3d.forward = conv_spy
    try:
        seen, loss = count_native(lambda: forward_backward(twin, shape, dtype))
    finally:
        torch.nn.Conv3d.forward = orig_conv
    assert torch.isfinite(loss) and loss.dtype == torch.float32
    assert seen["gn_fwd"] == [code] * 18 and seen["pool_fwd"] == [code] * 4 and seen["up_fwd"] == [code] * 4
    assert seen["gn_bwd"] == [code] * 18 and seen["pool_bwd"] == [code] * 4 and seen["up_bwd"] == [code] * 4
    assert not seen["gn_infer"]
    assert len(convs) == 19 and convs[0] == (torch.float32, True), convs
    assert all(c == (dtype, True) for c in convs[1:]), convs
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())
               for p in model.parameters())


@pytest.mark.parametrize("name", DTYPES)
def test_default_twin_under_autocast_keeps_todays_fallback(name):
    model = seeded_model().cuda()
    twin = trainable_ndhwc(model)
    seen, _ = count_native(lambda: forward_backward(twin, SHAPES[0], DTYPES[name]))
    assert set(sum(seen.values(), [])) <= {_native.DTYPE_F32}, seen


def gradient_errors(net, model, shape, dtype):
    model.zero_grad()
    forward_backward(net, shape, dtype)
    out = {}
    for n, p in model.named_parameters():
        g64 = reference_gradients(shape)[n]
        g = p.grad.cpu().numpy().astype(np.float64) / LOSS_SCALE
        out[n] = float(np.linalg.norm(g - g64) / np.linalg.norm(g64))
    return out


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_against_fp64(name, shape):
    """Per parameter: relative error of the half twin <= 4 x that of the plain model under the framework's autocast
    (both half-precision evaluations that differ in where they round; the margin is the fp32 test's).  Loss scaled
    by 2^10 in both runs so that fp16 gradients do not underflow; the fp64 reference is unscaled."""
    dtype = DTYPES[name]
    plain = seeded_model().cuda()
    e_plain = gradient_errors(plain, plain, shape, dtype)
    model = seeded_model().cuda()
    e_twin = gradient_errors(trainable_ndhwc(model, precision=name), model, shape, dtype)
    worst = max(e_twin, key=lambda n: e_twin[n] / e_plain[n])
    print(f"{name} {shape}: max rel. gradient error twin {max(e_twin.values()):.3e}, plain autocast "
          f"{max(e_plain.values()):.3e}; worst ratio {e_twin[worst] / e_plain[worst]:.2f} at {worst}")
    for n in e_twin:
        print(f"  {n}: twin {e_twin[n]:.3e} plain {e_plain[n]:.3e} ratio {e_twin[n] / e_plain[n]:.2f}")
    for n in e_twin:
        assert e_twin[n] <= 4 * e_plain[n], (n, e_twin[n], e_plain[n])


def make_scaler(name):
    return torch.amp.GradScaler("cuda", init_scale=1024.0) if name == "fp16" else None


def three_steps(name, shape):
    model = seeded_model().cuda()
    twin = trainable_ndhwc(model, precision=name)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    scaler = make_scaler(name)
    x, y, mask = (t.cuda() for t in batch(shape))
    losses = [train_step(twin, opt, SignalPreservingLoss(), x, y, mask, scaler=scaler, precision=name)
              for _ in range(3)]
    return model, twin, opt, scaler, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("name", DTYPES)
def test_three_steps_a_checkpoint_and_an_overflow(name, tmp_path):
    """fp16 with ``GradScaler(init_scale=1024)``, bf16 without.  Bit for bit: the first loss (a forward pass of
    deterministic kernels).  Then, fp16 only, one more step whose target holds an inf: the loss and with it every
    gradient is non-finite, the scaler must see that -- no parameter changes and the scale is halved."""
    before = {k: v.clone() for k, v in seeded_model().state_dict().items()}
    model, twin, opt, scaler, a = three_steps(name, SHAPES[1])
    _, _, _, _, b = three_steps(name, SHAPES[1])
    print(f"{name} losses:", a, b)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert a[0].tobytes() == b[0].tobytes()
    state = model.state_dict()
    assert all(v.dtype == before[k].dtype for k, v in state.items())
    assert sum(not torch.equal(v.cpu(), before[k]) for k, v in state.items()) == len(state)
    path = tmp_path / "ckpt.pt"
    torch.save(state, path)
    loaded, _ = inference.load_model(str(path))
    assert list(loaded.state_dict().keys()) == list(UNet().state_dict().keys())
    for k, v in state.items():
        assert torch.equal(loaded.state_dict()[k].cpu(), v.cpu())
    if name != "fp16":
        return
    scale = scaler.get_scale()
    x, y, mask = (t.cuda() for t in batch(SHAPES[1]))
    y[0, 0, 3, 4, 5] = float("inf")
    held = [p.detach().clone() for p in model.parameters()]
    loss = train_step(twin, opt, SignalPreservingLoss(), x, y, mask, scaler=scaler, precision=name)
    assert not torch.isfinite(loss)
    for p, h in zip(model.parameters(), held):
        assert torch.equal(p.detach().view(torch.int32), h.view(torch.int32))
    assert scale >= 2.0 and scaler.get_scale() == scale / 2


def test_fp32_precision_is_todays_step():
    x, y, mask = (t.cuda() for t in batch(SHAPES[0]))
    losses = []
    for kwargs in ({}, {"precision": "fp32"}):
        model = seeded_model().cuda()
        twin = trainable_ndhwc(model, **kwargs)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        losses.append(train_step(twin, opt, SignalPreservingLoss(), x, y, mask, **kwargs).cpu().numpy())
    assert losses[0].tobytes() == losses[1].tobytes() and np.isfinite(losses[0])
