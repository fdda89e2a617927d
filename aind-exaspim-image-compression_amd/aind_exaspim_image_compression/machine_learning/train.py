"""One BM4DNet training step on the device, on the layout the fast convolutions use.

The reference's ``Trainer`` (machine_learning/train.py) runs ``model`` in the framework's default layout with the
torch expression of the loss.  Here ``trainable_ndhwc(model)`` gives the same network, with the same Parameters,
in NDHWC with GroupNorm + LeakyReLU, max-pool and up-sampling running forward AND backward as ``libexabm4d``
kernels, and ``train_step`` is the reference's step (train.py:196-205, :285-320) in fp32 or, as the reference's
``Trainer`` runs it by default (``use_amp=True``), under fp16 / bf16 autocast: ``trainable_ndhwc(model,
precision=p)`` and ``train_step(..., precision=p)`` keep the three layers native on the half-width tensors the
autocast convolutions produce.  ``validate`` is the scoring half of ``Trainer.validate`` (train.py:224-283):
forward pass and loss per batch, the count-space metrics of every example in one device pass
(``metrics.evaluate_examples``), compression ratios, and the reference's aggregation into ``(loss, cratio,
score)``.  Not a port of ``Trainer``: data loading, the loop, logging and checkpoint files stay with the caller
(INTEGRATION.md).
"""
import copy

import numpy as np
import torch

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.inference import PRECISIONS, _fuse_norm_act, _miopen_defaults
from aind_exaspim_image_compression.machine_learning import metrics as _metrics
from aind_exaspim_image_compression.utils import img_util

CRATIO_CHUNK = (64, 64, 64)     # img_util.compute_cratio's patch_shape


def _check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, not {precision!r}")


def trainable_ndhwc(model, precision="fp32"):
    """An NDHWC (``channels_last_3d``) twin of ``model`` for training: its Parameters and buffers ARE the
    model's (the same objects), its (GroupNorm, LeakyReLU) pairs, ``MaxPool3d(2)`` and trilinear ``Upsample(2)``
    are the ``trainable=True`` modules of ``inference`` -- native forward and backward for fp32 CUDA tensors
    under gradients, the framework's modules for everything else (CPU, half precision, other shapes).

    So an optimiser built on ``model.parameters()`` trains the twin, ``model.state_dict()`` keeps the reference's
    keys, and a checkpoint written from ``model`` loads through ``inference.load_model``.  The twin's own
    ``state_dict`` keys are NOT the model's: save ``model``.

    Like ``inference.tune_model`` this CHANGES THE CALLER'S MODEL: its weights are converted to
    ``channels_last_3d`` in place (values and ``state_dict`` unchanged; the plain model keeps working, on the
    NDHWC solvers).  Module flags are copied, not shared: call ``.train()`` / ``.eval()`` on the twin you run.
    Convolutions keep their bias on this path, and every norm pair writes a new tensor.

    ``precision`` (one of ``inference.PRECISIONS``): ``"fp16"`` / ``"bf16"`` build the twin for a step under
    ``torch.autocast`` of that dtype (``train_step(..., precision=...)``): its modules also take the half-width
    NDHWC tensors the autocast convolutions hand over, forward and backward, and save their activations in that
    dtype.  The Parameters stay fp32 and shared, ``model.state_dict()`` stays the checkpoint.  With the default
    ``"fp32"`` nothing changes: a caller's own autocast around that twin falls back to the framework as before."""
    _check_precision(precision)
    _miopen_defaults()
    model.to(memory_format=torch.channels_last_3d)
    memo = {id(t): t for t in list(model.parameters()) + list(model.buffers())}
    twin = copy.deepcopy(model, memo)
    return _fuse_norm_act(twin, half=PRECISIONS[precision] is not None, trainable=True)


def train_step(net, optimizer, criterion, x, y, fg_mask, scaler=None, precision="fp32"):
    """Forward, loss, backward, optimiser step (reference train.py:196-205): ``net(x)`` against ``y`` under
    ``criterion(pred, y, fg_mask)``.  ``scaler``: an optional ``torch.amp.GradScaler`` used as the reference
    uses it (scale, step, update).  Returns the loss as a detached device tensor -- ``.item()``, and with it
    the host synchronisation, is the caller's decision.

    ``precision`` (one of ``inference.PRECISIONS``; anything else is a ``ValueError`` before any device work):
    ``"fp16"`` / ``"bf16"`` run the forward pass and the criterion under ``torch.autocast("cuda", dtype=...)``,
    the reference's ``forward_pass``; pass the twin ``trainable_ndhwc(model, precision=...)`` of the same
    precision to keep its layers native.  fp16 wants a ``GradScaler`` (its gradients underflow without one, and
    the scaler skips the step whose gradients overflowed -- the kernels pass inf / NaN on, they do not hide
    them); bf16 has fp32's exponent range and needs none.  The loss is evaluated in fp32 either way."""
    _check_precision(precision)
    amp_dtype = PRECISIONS[precision]
    with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype is not None):
        pred = net(x)
        loss = criterion(pred, y, fg_mask)
    optimizer.zero_grad()
    if scaler is not None:
        scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
    else:
        loss.backward()
        optimizer.step()
    return loss.detach()


def _net_device(net, x):
    """Where the batch is scored: the network's device, or for a network without parameters the batch's (when it
    is on a GPU already) or the current one."""
    for p in getattr(net, "parameters", lambda: [])():
        return p.device
    if x.is_cuda:
        return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _counts(ctx, transform, t, dev):
    """(B, 1, z, y, x) values of the transform domain -> (B, z, y, x) uint16 counts, on the device (the
    reference's ``transform.inverse`` of every example: train.py:335, :367-368)."""
    if t.dim() != 5 or t.shape[1] != 1:
        raise ValueError(f"validate expects (B, 1, z, y, x) tensors, got {tuple(t.shape)}")
    src = t.detach().to(torch.float32).contiguous()
    out = torch.empty((t.shape[0],) + tuple(t.shape[2:]), dtype=torch.uint16, device=dev)
    transform.inverse_device(ctx, src, out, src.numel())
    return out


def _entropy_cratio(img):
    from aind_exaspim_image_compression import evaluate
    return evaluate._cratio(img, None)


def _cratios(ctx, pred_counts, codec):
    """``img_util.compute_cratio`` of every example of (B, z, y, x) uint16 counts on the device."""
    b, shape = pred_counts.shape[0], tuple(int(s) for s in pred_counts.shape[1:])
    chunk = tuple(min(c, s) for c, s in zip(CRATIO_CHUNK, shape))
    if hasattr(codec, "encode_device") and shape[0] % chunk[0] == 0:
        # the examples stacked along z: whole chunks per example, numbered in raster order
        enc = codec.encode_device(ctx, pred_counts, (b * shape[0],) + shape[1:], chunk, want_bytes=False)
        sizes = np.asarray(enc.sizes, dtype=np.uint64).reshape(b, -1).sum(axis=1)
        raw_bytes = 2 * shape[0] * shape[1] * shape[2]
        return [round(raw_bytes / int(s), 2) for s in sizes]
    host = pred_counts.cpu().numpy()
    if codec is None:
        return [_entropy_cratio(img) for img in host]
    return [img_util.compute_cratio(img, codec) for img in host]


def validate(net, batches, criterion, transform, codec=None, precision="fp32", checkpoint_weights=None, pct=0.1):
    """Score ``net`` on a validation set: the reference's ``Trainer.validate`` (train.py:224-283) without its
    writer.  ``batches`` yields ``(x, y, raw, fg_mask)`` -- x, y and fg_mask (B, 1, z, y, x) tensors in the
    transform domain as the training set yields them, raw the noisy counts of the same shape (uint16 or float32;
    other types are converted to float32) -- as tensors or numpy arrays, on any device.

    Per batch, under ``torch.inference_mode()``: ``net(x)`` and ``criterion(pred, y, fg_mask)`` (under autocast
    for ``precision`` "fp16" / "bf16", as in ``train_step``; pass the twin of that precision), prediction and
    target back to uint16 counts with ``transform.inverse_device``, ``metrics.evaluate_examples`` on those device
    buffers (foreground: ``fg_mask > 0.5``), and one compression ratio per example as
    ``img_util.compute_cratio(pred, codec)`` gives it: a device codec (one with ``encode_device``, e.g.
    ``ExacCodec(2)``) codes the stacked predictions in one call, any other codec gets the downloaded predictions,
    ``codec=None`` reports ``evaluate``'s entropy proxy.

    Returns ``{"loss": mean of the batch losses, "cratio": median ratio, "score": checkpoint_score(metrics,
    cratio, checkpoint_weights), "metrics": the mean of every metric over all examples, "n": examples}``;
    without examples ``loss`` and ``cratio`` are NaN and ``score`` is None.  The network runs in eval mode and gets
    its mode back.  An unknown ``precision`` is a ``ValueError`` before any device work.  The DataLoader, logging,
    checkpoint files and the loop that decides when to validate stay with the caller."""
    _check_precision(precision)
    amp_dtype = PRECISIONS[precision]
    losses, cratios, rows = [], [], []
    was_training = getattr(net, "training", False)
    if hasattr(net, "eval"):
        net.eval()
    try:
        with torch.inference_mode():
            for x, y, raw, fg_mask in batches:
                x = torch.as_tensor(x)
                dev = _net_device(net, x)
                x, y, fg_mask = (torch.as_tensor(t).to(dev) for t in (x, y, fg_mask))
                raw = torch.as_tensor(raw).to(dev)
                if raw.dtype not in (torch.uint16, torch.float32):
                    raw = raw.to(torch.float32)
                if x.dim() != 5 or any(t.shape != x.shape for t in (y, raw, fg_mask)):
                    raise ValueError("validate expects x, y, raw and fg_mask of one (B, 1, z, y, x) shape")
                with torch.autocast("cuda", dtype=amp_dtype, enabled=amp_dtype is not None):
                    pred = net(x)
                    loss = criterion(pred, y, fg_mask)
                losses.append(loss.item())
                ctx = _native.context(dev.index or 0)
                with torch.cuda.device(dev):
                    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                    try:
                        pred_counts = _counts(ctx, transform, pred, dev)
                        target_counts = _counts(ctx, transform, y, dev)
                    finally:
                        ctx.reset_stream()
                    # ends with a synchronisation of torch's stream: the counts are complete for the codec
                    rows.extend(_metrics.evaluate_examples(pred_counts, raw[:, 0], target_counts, fg_mask[:, 0],
                                                           pct=pct))
                    cratios.extend(_cratios(ctx, pred_counts, codec))
    finally:
        if was_training and hasattr(net, "train"):
            net.train()
    if not rows:
        return {"loss": float("nan"), "cratio": float("nan"), "score": None, "metrics": {}, "n": 0}
    loss = float(np.mean(losses))
    cratio = float(np.median(cratios))
    agg = {k: float(np.mean([row[k] for row in rows])) for k in rows[0]}
    return {"loss": loss, "cratio": cratio, "score": _metrics.checkpoint_score(agg, cratio, checkpoint_weights),
            "metrics": agg, "n": len(rows)}
