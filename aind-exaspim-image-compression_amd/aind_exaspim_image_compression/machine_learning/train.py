"""One BM4DNet training step on the device, on the layout the fast convolutions use.

The reference's ``Trainer`` (machine_learning/train.py) runs ``model`` in the framework's default layout with the
torch expression of the loss.  Here ``trainable_ndhwc(model)`` gives the same network, with the same Parameters,
in NDHWC with GroupNorm + LeakyReLU, max-pool and up-sampling running forward AND backward as ``libexabm4d``
kernels, and ``train_step`` is the reference's step (train.py:196-205, :285-320) in fp32 or, as the reference's
``Trainer`` runs it by default (``use_amp=True``), under fp16 / bf16 autocast: ``trainable_ndhwc(model,
precision=p)`` and ``train_step(..., precision=p)`` keep the three layers native on the half-width tensors the
autocast convolutions produce.  Not a port of ``Trainer``: data loading, validation, logging and checkpoint
selection stay with the caller.
"""
import copy

import torch

from aind_exaspim_image_compression.inference import PRECISIONS, _fuse_norm_act, _miopen_defaults


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
