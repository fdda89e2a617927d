"""Loss functions for signal-preserving denoising (drop-in for the reference ``machine_learning/losses.py``).

Same names, defaults, attributes and ``forward(pred, target, fg_mask)`` as the reference (losses.py:10-84).
What differs is where a training step's loss is evaluated: for contiguous fp32 CUDA tensors of equal shape the
value and its gradient are one pass each of ``libexabm4d`` (csrc/nn_grad_kernels.hip) -- every element in fp64,
fp64 partial sums combined in a fixed order, the result a one-element device tensor, no host synchronisation --
instead of the six elementwise kernels and six temporaries of the torch expression.  Everything else (CPU
tensors, other dtypes, masks that broadcast) evaluates the reference's expression.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from aind_exaspim_image_compression import _native

_MASK_BYTES = {torch.float32: 4, torch.uint8: 1, torch.bool: 1}


def charbonnier(diff, eps=1e-3):
    """The Charbonnier penalty ``sqrt(diff^2 + eps^2)``, elementwise: a smooth approximation of ``|diff|``."""
    return torch.sqrt(diff * diff + eps * eps)


def _same_dense_layout(tensors):
    """All contiguous, or all dense NDHWC: storage order then pairs the same elements in every tensor."""
    if all(t.is_contiguous() for t in tensors):
        return True
    return all(t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d) for t in tensors)


class _CharbonnierLossFn(torch.autograd.Function):
    """``mean((1 + w m) sqrt((pred - target)^2 + eps^2))`` and its gradient through ``libexabm4d``."""

    @staticmethod
    def forward(ctx, pred, target, mask, fg_weight, eps):
        lib = _native.lib()
        nctx = _native.context(pred.device.index or 0)
        need = int(lib.exabm4d_charbonnier_workspace_bytes())
        ws = torch.empty(need, dtype=torch.uint8, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        nctx.charbonnier_loss(torch.cuda.current_stream(pred.device).cuda_stream, pred, target, mask,
                              _MASK_BYTES[mask.dtype], pred.numel(), fg_weight, eps, ws, need, loss)
        ctx.save_for_backward(pred, target, mask)
        ctx.fg_weight, ctx.eps = fg_weight, eps
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        pred, target, mask = ctx.saved_tensors
        g = grad_loss.to(dtype=torch.float32).contiguous()       # a device scalar: under a GradScaler it is not 1
        dpred = torch.empty_like(pred)                            # dense like pred, same strides
        _native.context(pred.device.index or 0).charbonnier_loss_bwd(
            torch.cuda.current_stream(pred.device).cuda_stream, pred, target, mask, _MASK_BYTES[mask.dtype],
            pred.numel(), ctx.fg_weight, ctx.eps, g, dpred)
        return (dpred if ctx.needs_input_grad[0] else None, -dpred if ctx.needs_input_grad[1] else None,
                None, None, None)


class SignalPreservingLoss(nn.Module):
    """Foreground-weighted Charbonnier loss (reference losses.py:29-84): ``mean((1 + fg_weight * fg_mask) *
    charbonnier(pred - target, eps))``.  Upweights foreground voxels so that sparse, bright neurites are not
    drowned out by the background; operates in the transform domain.

    Attributes
    ----------
    fg_weight : float
        Extra weight on foreground voxels (0: a plain Charbonnier mean).
    eps : float
        Charbonnier smoothing constant.
    """

    def __init__(self, fg_weight=20.0, eps=1e-3):
        super().__init__()
        self.fg_weight = float(fg_weight)
        self.eps = float(eps)

    @staticmethod
    def _device_path(pred, target, fg_mask):
        return (pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
                and fg_mask.dtype in _MASK_BYTES and pred.numel() > 0
                and target.device == pred.device and fg_mask.device == pred.device
                and target.shape == pred.shape and fg_mask.shape == pred.shape
                and not fg_mask.requires_grad
                and _same_dense_layout((pred, target, fg_mask)))

    def forward(self, pred, target, fg_mask):
        """Scalar loss of a prediction and a target in the transform domain and a 0/1 foreground mask of the
        same shape.  Contiguous fp32 CUDA tensors of equal shape and layout (row-major or NDHWC; the mask fp32,
        uint8 or bool): the device kernels, result a 0-d fp32 CUDA tensor.  Otherwise the torch expression."""
        if self._device_path(pred, target, fg_mask):
            return _CharbonnierLossFn.apply(pred, target, fg_mask, self.fg_weight, self.eps)
        weight = 1.0 + self.fg_weight * fg_mask
        return (weight * charbonnier(pred - target, self.eps)).mean()
