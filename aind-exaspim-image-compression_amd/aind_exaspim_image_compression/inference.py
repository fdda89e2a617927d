"""GPU-resident tiled BM4DNet inference (drop-in for the reference ``inference.py``).

Same functions, signatures, defaults and return types as the reference
(``predict`` inference.py:28, ``predict_patch`` :119, ``load_model`` :255,
``build_volume_transform`` :302, helpers :178-252, :340-380).  What differs is where the work
happens: the reference transforms the volume with numpy, gathers patches with a thread pool,
copies every batch to and from the device and adds 8000 patches into host accumulators in a
Python loop (hot loops 1-2 of SURVEY.md section 3-A).  Here the volume is uploaded once; the
intensity transform, patch gather + zero padding, trim + overlap-add and the final
normalise -> inverse transform -> rint -> uint16 are HIP kernels of ``libexabm4d.so`` working on
buffers that stay in HBM, and only the uint16 result comes back.  The U-Net itself is PyTorch-ROCm.

Reference quirk kept on purpose (inference.py:91-103): the first ``trim``
voxels along every axis receive zero weight and come out as ``transform.inverse(0)``.
"""
import contextlib
import itertools
import os
import time

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from aind_exaspim_image_compression import _native
from aind_exaspim_image_compression.machine_learning.transforms import (
    build_transform,
    estimate_offset,
    with_offset,
)
from aind_exaspim_image_compression.machine_learning.unet3d import N2V2UNet, UNet

# predict(precision=...): the autocast dtype of the forward passes (None: fp32, no autocast)
PRECISIONS = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}
# element types of libexabm4d's NDHWC entries; the half-width ones only for a reduced-precision shadow's modules
_NATIVE_DTYPES = {torch.float32: _native.DTYPE_F32, torch.float16: _native.DTYPE_F16,
                  torch.bfloat16: _native.DTYPE_BF16}


def _native_dtype(dtype, half):
    """The libexabm4d element-type code for tensors of ``dtype``, or None where the NDHWC modules fall back."""
    code = _NATIVE_DTYPES.get(dtype)
    return code if code == _native.DTYPE_F32 or half else None


def _model_device(model):
    try:
        dev = next(model.parameters()).device
    except (StopIteration, AttributeError):
        dev = None
    if dev is None or dev.type != "cuda":
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    return dev


_MIOPEN_DONE = False


def _miopen_defaults():
    """Once per process, before its first convolution (``predict`` / ``load_model`` call it): make MIOpen
    pick the tuned solvers for the BM4DNet U-Net without a search.
      * a per-user MIOpen user-db directory (``$XDG_CACHE_HOME/exabm4d/miopen/torch-<version>``) seeded with
        the find-db records shipped in ``miopen_db/`` (27 KB of text MIOpen wrote during exhaustive searches
        on an MI355X, fp32, fp16 and bf16) -- unless the caller already chose ``MIOPEN_USER_DB_PATH``; searches the caller
        runs later (``tune_model``) persist there too, so they are paid once per machine, not per process;
      * ``MIOPEN_FIND_MODE=2`` (FAST) unless the caller set the variable: a find-db hit selects the recorded
        solver at once, a miss falls back to heuristics instead of timing every solver (17 s per process
        for this network in the default mode).
    ``EXABM4D_MIOPEN_DEFAULTS=0`` leaves MIOpen's environment alone.  Measured (tools/dbg/miopen_cache_probe.sh,
    U-Net forward 32 x 64^3 fp32): with the records first call 0.1 s, then 68 ms (51 TFLOP/s); without them
    and without this function 15 s, then 116 ms (30 TFLOP/s)."""
    global _MIOPEN_DONE
    if _MIOPEN_DONE:
        return
    _MIOPEN_DONE = True
    if os.environ.get("EXABM4D_MIOPEN_DEFAULTS", "1") == "0":
        return
    if "MIOPEN_USER_DB_PATH" not in os.environ:
        import shutil
        base = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"),
                            "exabm4d", "miopen", "torch-" + torch.__version__.replace("+", "_"))
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "miopen_db")
        try:
            os.makedirs(os.path.join(base, "db"), exist_ok=True)
            os.makedirs(os.path.join(base, "kernels"), exist_ok=True)
            for name in os.listdir(src):
                dst = os.path.join(base, "db", name)
                if name.endswith(".txt") and not os.path.exists(dst):
                    shutil.copyfile(os.path.join(src, name), dst)
            os.environ["MIOPEN_USER_DB_PATH"] = os.path.join(base, "db")
            os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(base, "kernels"))
        except OSError:
            pass                                   # read-only home: MIOpen's own defaults, FAST mode below
    os.environ.setdefault("MIOPEN_FIND_MODE", "2")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _as_ndhwc(t):
    """``t`` itself when its memory is dense NDHWC, else such a copy (a gradient arrives in any layout)."""
    return t.contiguous(memory_format=torch.channels_last_3d)


def _grad_as(dy, dtype):
    """The incoming gradient as a dense NDHWC tensor of the forward's ``dtype`` (autograd may hand over another)."""
    return _as_ndhwc(dy if dy.dtype == dtype else dy.to(dtype))


class _GroupNormLeakyReLUFn(torch.autograd.Function):
    """``LeakyReLU(GroupNorm(x))`` on an fp32, fp16 or bf16 NDHWC tensor with both directions in ``libexabm4d``
    (csrc/nn_kernels.hip forward, which also writes the (mean, rstd) it used; csrc/nn_grad_kernels.hip
    backward).  Out of place: the backward reads the input and the output.  ``code``: the element-type code of
    ``x``; x, y (both saved) and dx are in x's dtype, weight, bias, (mean, rstd) and their gradients fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, slope, code=_native.DTYPE_F32):
        b, c = int(x.shape[0]), int(x.shape[1])
        spatial = int(x.shape[2]) * int(x.shape[3]) * int(x.shape[4])
        need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(b, spatial, c, groups))
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x, memory_format=torch.channels_last_3d)
        stats = torch.empty((b, groups, 2), dtype=torch.float32, device=x.device)
        _native.context(x.device.index or 0).groupnorm_lrelu_ndhwc_train(
            _stream(x), x, y, b, spatial, c, groups, weight, bias, eps, slope, ws, need, stats, dtype=code)
        ctx.save_for_backward(x, y, weight, stats)
        ctx.groups, ctx.slope, ctx.code = groups, slope, code
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, weight, stats = ctx.saved_tensors
        b, c = int(x.shape[0]), int(x.shape[1])
        spatial = int(x.shape[2]) * int(x.shape[3]) * int(x.shape[4])
        dy = _grad_as(dy, x.dtype)
        dx = torch.empty_like(x, memory_format=torch.channels_last_3d)
        want_w = weight is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dgamma = torch.empty_like(weight) if want_w else None
        dbeta = torch.empty_like(weight) if want_w else None
        need = int(_native.lib().exabm4d_groupnorm_lrelu_bwd_workspace_bytes(b, spatial, c, ctx.groups))
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _native.context(x.device.index or 0).groupnorm_lrelu_bwd_ndhwc(
            _stream(x), x, y, dy, dx, b, spatial, c, ctx.groups, weight, stats, ctx.slope, dgamma, dbeta, ws, need,
            dtype=ctx.code)
        return dx, dgamma, dbeta, None, None, None, None


class _MaxPool2Fn(torch.autograd.Function):
    """``MaxPool3d(2)`` on an NDHWC tensor of element type ``code``; the backward re-reads the input's windows
    instead of storing indices (csrc/nn_grad_kernels.hip: torch's choice among ties and NaNs)."""

    @staticmethod
    def forward(ctx, x, code=_native.DTYPE_F32):
        b, c, d, h, w = (int(v) for v in x.shape)
        y = torch.empty((b, c, d // 2, h // 2, w // 2), dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last_3d)
        _native.context(x.device.index or 0).maxpool2_ndhwc(_stream(x), x, y, b, d, h, w, c, dtype=code)
        ctx.save_for_backward(x)
        ctx.code = code
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        b, c, d, h, w = (int(v) for v in x.shape)
        dx = torch.empty_like(x, memory_format=torch.channels_last_3d)
        _native.context(x.device.index or 0).maxpool2_bwd_ndhwc(_stream(x), x, _grad_as(dy, x.dtype), dx, b, d, h, w,
                                                                c, dtype=ctx.code)
        return dx, None


class _Upsample2Fn(torch.autograd.Function):
    """Trilinear x2 up-sampling (align_corners) on an NDHWC tensor of element type ``code`` and its transpose."""

    @staticmethod
    def forward(ctx, x, code=_native.DTYPE_F32):
        b, c, d, h, w = (int(v) for v in x.shape)
        y = torch.empty((b, c, 2 * d, 2 * h, 2 * w), dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last_3d)
        _native.context(x.device.index or 0).upsample2_trilinear_ndhwc(_stream(x), x, y, b, d, h, w, c, dtype=code)
        ctx.dims = (b, c, d, h, w)
        ctx.code, ctx.dtype = code, x.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        b, c, d, h, w = ctx.dims
        dy = _grad_as(dy, ctx.dtype)
        dx = torch.empty((b, c, d, h, w), dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last_3d)
        _native.context(dy.device.index or 0).upsample2_trilinear_bwd_ndhwc(_stream(dy), dy, dx, b, d, h, w, c,
                                                                            dtype=ctx.code)
        return dx, None


def _trainable_input(x, half=False):
    """What the training path of the NDHWC modules takes: gradients on, a CUDA NDHWC tensor that is fp32 or, for a
    module built with ``half=True``, fp16 / bf16.  Returns the tensor's element-type code, or None."""
    if not (torch.is_grad_enabled() and x.is_cuda and x.dim() == 5
            and x.is_contiguous(memory_format=torch.channels_last_3d)):
        return None
    return _native_dtype(x.dtype, half)


class FusedGroupNormLeakyReLU(torch.nn.Module):
    """``GroupNorm`` followed by ``LeakyReLU`` as ONE module for inference on NDHWC tensors: the pair of the
    reference's ``DoubleConv`` (unet3d.py:137-208) through ``exabm4d_groupnorm_lrelu_ndhwc_dev`` -- statistics,
    normalisation and activation in two passes over the layout MIOpen's convolutions produce, in place on the
    convolution's output (``inplace``) or into a new tensor.  PyTorch's own GroupNorm wants NCDHW: per layer a
    layout copy in, statistics, apply, the activation and a layout copy back (45 % of the forward's kernel time).
    Falls back to the framework's two modules for anything the kernels do not take (training, other dtypes /
    layouts / channel counts); the fallback never writes into its input.  ``trainable=True`` adds a path for
    training: with gradients enabled, an fp32 CUDA NDHWC input of a supported shape runs ``_GroupNormLeakyReLUFn``,
    whose backward is ``libexabm4d``'s too (out of place; needs ``negative_slope > 0`` and the convolution's bias
    left in the convolution); with ``half=True`` as well, so does the fp16 / bf16 tensor an autocast convolution
    hands over (saved tensors and dx in that dtype, gamma, beta and their gradients fp32); with ``half=False``
    half-precision tensors under gradients fall back."""

    def __init__(self, norm, act, conv_bias=None, half=False, inplace=True, trainable=False):
        """``conv_bias``: the bias of the convolution in front, taken over from it (the caller sets that
        convolution's ``bias`` to None): added inside the kernels instead of in a pass of its own.
        ``half``: also take fp16 / bf16 tensors (the half-width kernels; gamma, beta and the bias stay fp32) --
        for the shadow ``predict(precision="fp16" | "bf16")`` builds; otherwise those fall back as before.
        ``inplace`` (default, as for the U-Net's pairs): the kernels overwrite their input -- only for an input
        nothing else reads afterwards, a convolution's fresh output; ``inplace=False``: the result goes to a new
        ``channels_last_3d`` tensor and the input is left as it was (``_fuse_norm_act`` decides per pair)."""
        super().__init__()
        self.norm, self.act = norm, act
        self.conv_bias = conv_bias
        self.half = half
        self.inplace = inplace
        self.trainable = trainable
        self._ws = None

    @property
    def native_channels(self):
        """Whether the kernels take this norm's channels: C % 4 == 0, (C / G) % 4 == 0, 256 % (C / 4) == 0 and
        G <= 32 (see include/exabm4d.h)."""
        c, g = self.norm.num_channels, self.norm.num_groups
        return c % 4 == 0 and (c // g) % 4 == 0 and 256 % (c // 4) == 0 and g <= 32

    def forward(self, x):
        n = self.norm
        code = _trainable_input(x, self.half) if self.trainable else None
        if (code is not None and self.native_channels and x.shape[0] <= 65535
                and n.affine and self.conv_bias is None and self.act.negative_slope > 0):
            return _GroupNormLeakyReLUFn.apply(x, n.weight, n.bias, n.num_groups, n.eps, self.act.negative_slope,
                                               code)
        code = _native_dtype(x.dtype, self.half)
        fused = (not self.training and x.is_cuda and code is not None and x.dim() == 5
                 and x.is_contiguous(memory_format=torch.channels_last_3d) and not torch.is_grad_enabled()
                 and self.native_channels and x.shape[0] <= 65535)
        if not fused:
            if self.conv_bias is not None:
                x = x + self.conv_bias.view(1, -1, 1, 1, 1)
            return self.act(self.norm(x))
        b, c = int(x.shape[0]), int(x.shape[1])
        spatial = int(x.shape[2]) * int(x.shape[3]) * int(x.shape[4])
        need = int(_native.lib().exabm4d_groupnorm_workspace_bytes(b, spatial, c, n.num_groups))
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        y = x if self.inplace else torch.empty_like(x, memory_format=torch.channels_last_3d)
        ctx = _native.context(x.device.index or 0)
        ctx.groupnorm_lrelu_ndhwc(torch.cuda.current_stream(x.device).cuda_stream, x, y, b, spatial, c,
                                  n.num_groups, n.weight, n.bias, n.eps, self.act.negative_slope,
                                  self._ws, need, self.conv_bias, dtype=code)
        return y


def _all_equal(v, want):
    return all(x == want for x in (v if isinstance(v, (tuple, list)) else (v,)))


class _ResampleNDHWC(torch.nn.Module):
    """The U-Net's ``MaxPool3d(2)`` and ``Upsample(scale_factor=2, mode="trilinear", align_corners=True)`` on
    NDHWC tensors through ``libexabm4d`` (csrc/nn_kernels.hip: a float4 of channels per thread).  PyTorch's own
    kernels for the two walk an NDHWC tensor through generic strides (3.8 ms per call on this U-Net's tensors);
    anything else -- other parameters, layouts, dtypes, training -- runs ``inner`` on an NCDHW copy.  ``half``: as
    for ``FusedGroupNormLeakyReLU``, fp16 / bf16 tensors run natively too.  ``trainable=True``: with gradients
    enabled, an fp32 CUDA NDHWC input -- with ``half=True`` also an fp16 / bf16 one -- runs ``_MaxPool2Fn`` /
    ``_Upsample2Fn`` (native forward and backward)."""

    def __init__(self, inner, half=False, trainable=False):
        super().__init__()
        self.inner = inner
        self.half = half
        self.trainable = trainable
        m = inner
        if isinstance(m, torch.nn.MaxPool3d):
            ok = (_all_equal(m.kernel_size, 2) and _all_equal(m.stride if m.stride is not None else m.kernel_size, 2)
                  and _all_equal(m.padding, 0) and _all_equal(m.dilation, 1) and not m.ceil_mode
                  and not m.return_indices)
            self.kind = "pool" if ok else None
        elif isinstance(m, torch.nn.Upsample):
            ok = (m.mode == "trilinear" and m.align_corners is True and m.size is None
                  and m.scale_factor is not None and _all_equal(m.scale_factor, 2))
            self.kind = "up" if ok else None
        else:
            self.kind = None

    def forward(self, x):
        code = _trainable_input(x, self.half) if self.trainable and self.kind is not None else None
        if code is not None and x.shape[1] % 4 == 0:
            if self.kind == "up":
                return _Upsample2Fn.apply(x, code)
            if min(x.shape[2:]) >= 2:
                return _MaxPool2Fn.apply(x, code)
        code = _native_dtype(x.dtype, self.half)
        native = (self.kind is not None and not self.training and not torch.is_grad_enabled() and x.is_cuda
                  and code is not None and x.dim() == 5 and x.shape[1] % 4 == 0
                  and x.is_contiguous(memory_format=torch.channels_last_3d)
                  and (self.kind == "up" or min(x.shape[2:]) >= 2))
        if not native:
            return self.inner(x.contiguous())
        b, c, d, h, w = (int(v) for v in x.shape)
        out_dims = (d // 2, h // 2, w // 2) if self.kind == "pool" else (2 * d, 2 * h, 2 * w)
        y = torch.empty((b, c) + out_dims, dtype=x.dtype, device=x.device, memory_format=torch.channels_last_3d)
        ctx = _native.context(x.device.index or 0)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if self.kind == "pool":
            ctx.maxpool2_ndhwc(stream, x, y, b, d, h, w, c, dtype=code)
        else:
            ctx.upsample2_trilinear_ndhwc(stream, x, y, b, d, h, w, c, dtype=code)
        return y


def _fuse_norm_act(module, half=False, trainable=False):
    """Replace every (GroupNorm, LeakyReLU) neighbour pair inside ``nn.Sequential`` containers of ``module`` by
    a ``FusedGroupNormLeakyReLU`` + ``Identity`` (same positions: the copy's parameters are the pair's), and
    put every ``MaxPool3d`` / ``Upsample`` behind ``_ResampleNDHWC``.  For the private copy ``_ndhwc_shadow`` makes;
    its ``state_dict`` keys are not the model's any more.  ``half``: the new modules take fp16 / bf16 too.
    ``trainable`` (``machine_learning.train.trainable_ndhwc``): the new modules get ``trainable=True``, every pair
    writes a new tensor and every convolution keeps its bias (its gradient is then the convolution's business).

    What the rewrite can see is the module tree, so it stays correct only where the tree tells the data flow:
      * a pair runs in place only right behind a ``Conv3d`` in the same container (a fresh output nobody else
        holds); at the head of a container, or behind a module that may return its input (``Identity``,
        ``Dropout`` in eval mode, ...), it writes a new tensor;
      * the convolution's bias moves into the fused kernels only when that ``Conv3d`` sits in ONE slot of the
        tree (one container, one name); a convolution that also appears elsewhere keeps its bias;
      * each module is rewritten once, however many slots share it.
    Not visible, so not accounted for: a custom ``forward`` that calls an element of a ``Sequential`` outside
    it (``self.block[0](x)``), forward hooks on the replaced modules, and functional ``F.group_norm`` /
    ``F.max_pool3d`` / ``F.interpolate`` calls (those run as the framework's, unchanged)."""
    slots = {}                                       # id(child) -> the (container, name) slots holding it
    for parent in module.modules():
        for name, child in parent._modules.items():
            if child is not None:
                slots.setdefault(id(child), set()).add((id(parent), name))
    for parent in list(module.modules()):            # unique modules; the wrappers made below are not revisited
        for name, child in list(parent._modules.items()):
            if isinstance(child, (torch.nn.MaxPool3d, torch.nn.Upsample)):
                setattr(parent, name, _ResampleNDHWC(child, half, trainable).train(parent.training))
        if not isinstance(parent, torch.nn.Sequential):
            continue
        for i in range(len(parent) - 1):
            a, b = parent[i], parent[i + 1]
            if isinstance(a, torch.nn.GroupNorm) and isinstance(b, torch.nn.LeakyReLU) and a.affine:
                conv = parent[i - 1] if i > 0 else None
                after_conv = isinstance(conv, torch.nn.Conv3d)
                bias = None
                if (not trainable and after_conv and conv.bias is not None
                        and conv.out_channels == a.num_channels and len(slots[id(conv)]) == 1):
                    bias, conv.bias = conv.bias, None             # added inside the fused kernels instead
                # (a new module starts in training mode)
                parent[i] = FusedGroupNormLeakyReLU(a, b, bias, half, inplace=after_conv and not trainable,
                                                    trainable=trainable).train(parent.training)
                parent[i + 1] = torch.nn.Identity().train(parent.training)
    return module


def _ndhwc_shadow(model, fuse=True, half=False):
    """An NDHWC (channels_last_3d) copy of an eval-mode fp32 module for the forward passes of one ``predict``
    call: MIOpen's implicit-GEMM solvers for NDHWC weights run this U-Net at 51 TFLOP/s against 30 for the
    default layout, and (``fuse``) its GroupNorm + LeakyReLU pairs run as the fused NDHWC kernels of
    ``libexabm4d`` instead of converting the layout there and back around PyTorch's GroupNorm.  The caller's
    model is not touched (52 MB copied per call); same fp32 arithmetic, results differ by summation order
    (tests at 2e-3 against the golden patch).  ``half``: for forward passes under an fp16 / bf16 autocast
    (``predict(precision=...)``): the parameters stay fp32, the fused modules also take the half-width tensors
    autocast's convolutions produce.  Any module may come in, not only this package's U-Nets: the rewrite
    writes in place and moves a convolution's bias only where the module tree shows that is safe, and what the
    tree cannot show is listed at ``_fuse_norm_act`` (tests/nn_zoo.py holds the models it is checked on)."""
    import copy
    shadow = copy.deepcopy(model).to(memory_format=torch.channels_last_3d)
    return _fuse_norm_act(shadow, half) if fuse else shadow


def tune_model(model):
    """Opt-in MIOpen tuning for the BM4DNet stage on MI355X: NDHWC weights + exhaustive solver
    search (``torch.backends.cudnn.benchmark``, process-wide).  U-Net forward, 32 x 64^3 fp32:
    116 -> 69 ms (tools/dbg/unet_variants.py); same fp32 arithmetic, results differ by summation
    order only (4e-6).  Both halves are needed -- NDHWC weights WITHOUT the search fall on a slow
    default solver -- and the search runs once per input shape, so this is for long jobs; it is
    not applied by default and ``predict`` itself never changes the caller's model."""
    torch.backends.cudnn.benchmark = True
    if isinstance(model, torch.nn.Module):
        model.to(memory_format=torch.channels_last_3d)
    return model


def quick_start(model):
    """Opt-in for ONE-OFF volumes on a fresh process: NDHWC weights + MIOpen's FAST find mode
    (``MIOPEN_FIND_MODE=2``, set here unless the caller set the variable; it must happen before the
    process runs its first convolution).  MIOpen's default find mode spends 17 s on the first U-Net
    batch of a process (kernel selection by timing); FAST mode picks by heuristics in 0.2 s.  Measured on
    an MI355X, U-Net forward 32 x 64^3 fp32 (tools/dbg/miopen_modes.py): default mode, default layout:
    first call 16.8 s, then 117 ms; FAST + NDHWC: first call 0.2 s, then 122 ms; FAST with the default
    layout falls on a slow solver (316 ms) -- hence both halves here.  For one 1024^3 volume (250
    batches), measured on a fresh process: 30.7 s against 43.5 s (tools/dbg/quick_start_1024.py); for long jobs ``tune_model`` (39 s search, then 70 ms) wins.
    Same fp32 arithmetic in all three; results differ by summation order only."""
    os.environ.setdefault("MIOPEN_FIND_MODE", "2")
    if isinstance(model, torch.nn.Module):
        model.to(memory_format=torch.channels_last_3d)
    return model


def _forward_plan(model, fast, amp_dtype):
    """How ``predict`` and ``predict_store`` run their forward passes: ``(run, loop_amp, call_amp)`` -- what to call
    on a batch, the context around the whole loop and the one around each call.  ``run`` is an NDHWC shadow of an
    eval-mode fp32 module under ``fast``, else ``model`` itself."""
    run = model
    shadowed = False
    if fast and isinstance(model, torch.nn.Module) and not model.training and \
            all(p.dtype == torch.float32 for p in model.parameters()) and any(True for _ in model.parameters()):
        run = _ndhwc_shadow(model, half=amp_dtype is not None)
        shadowed = True
    # the shadow's forward passes share one autocast region (its weights are cast once per call, not per batch);
    # a caller's module or callable gets autocast around each call
    amp = (lambda: torch.autocast("cuda", dtype=amp_dtype)) if amp_dtype is not None else contextlib.nullcontext
    loop_amp, call_amp = (amp, contextlib.nullcontext) if shadowed else (contextlib.nullcontext, amp)
    return run, loop_amp, call_amp


def predict(img, model, transform, batch_size=32, patch_size=64, overlap=12, trim=5,
            verbose=True, fast=True, precision="fp32"):
    """Denoise a 3-D image by overlapping-patch inference; returns uint16 counts.

    Parameters follow the reference (inference.py:28-67): ``img`` is a 3-D array (leading
    singleton axes are accepted), ``model`` a torch module (or any callable on a
    ``(B,1,P,P,P)`` float32 CUDA tensor), ``transform`` the IntensityTransform the model was
    trained with.  ``fast`` (not in the reference; default on): an eval-mode ``nn.Module`` runs its forward
    passes through an NDHWC copy of itself with MIOpen's tuned solvers (``_miopen_defaults``,
    ``_ndhwc_shadow``; fp32 throughout); ``fast=False`` calls ``model`` exactly as given.

    ``precision`` (not in the reference; default ``"fp32"``): ``"fp32"``, ``"fp16"`` or ``"bf16"``, the
    arithmetic of the network's forward passes; anything else is a ValueError.  ``"fp32"`` is the path
    described above.  ``"fp16"`` / ``"bf16"`` run the forward passes under ``torch.autocast`` of that dtype: the
    NDHWC copy's convolutions in half precision, its GroupNorm + LeakyReLU pairs, max-pools and up-samplings
    through the half-width kernels of ``libexabm4d`` (parameters fp32); with ``fast=False`` or a callable,
    autocast around each call only.  The input patches, the residual sum ``x + logits`` (autocast leaves the
    addition to type promotion: fp32), the network's output and the stitching stay fp32."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, not {precision!r}")
    amp_dtype = PRECISIONS[precision]
    _miopen_defaults()
    img = np.asarray(img)
    while img.ndim > 3:
        if img.shape[0] != 1:
            raise ValueError("predict expects a single 3-D volume")
        img = img[0]
    if img.ndim != 3:
        raise ValueError("predict expects a 3-D volume")
    shape = tuple(int(s) for s in img.shape)
    n = int(np.prod(shape))
    dev = _model_device(model)
    ctx = _native.context(dev.index or 0)
    run, loop_amp, call_amp = _forward_plan(model, fast, amp_dtype)

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        pbar = None
        ctx.set_stream(stream.cuda_stream)       # kernels and the model share one stream
        try:
            src_u16 = img.dtype == np.uint16
            host = np.ascontiguousarray(img if src_u16 else img.astype(np.float32))
            d_raw = torch.from_numpy(host.view(np.int16) if src_u16 else host).to(dev)
            vol = torch.empty(shape, dtype=torch.float32, device=dev)
            transform.forward_device(ctx, d_raw, vol, n, src_u16)          # inference.py:69
            del d_raw

            accum_pred = torch.zeros(shape, dtype=torch.float32, device=dev)   # inference.py:81-82
            accum_wgt = torch.zeros(shape, dtype=torch.float32, device=dev)
            starts = list(generate_patch_starts(_ShapeOnly((1, 1) + shape), patch_size, overlap))
            if verbose:
                from tqdm import tqdm
                pbar = tqdm(total=len(starts), desc="Denoise")
            batch = torch.empty((batch_size, 1, patch_size, patch_size, patch_size),
                                dtype=torch.float32, device=dev)
            with loop_amp():
                for b0 in range(0, len(starts), batch_size):
                    chunk = np.asarray(starts[b0:b0 + batch_size], dtype=np.int32)
                    nb = len(chunk)
                    ctx.tile_gather(vol, shape, chunk, patch_size, batch)      # inference.py:153-168
                    # A short last batch is run at full size (rows beyond nb hold the previous batch's
                    # patches and are dropped): MIOpen then sees ONE input shape per volume instead of
                    # paying a solver search -- seconds -- for the tail's.  Only for modules in eval mode,
                    # whose output rows do not depend on the rest of the batch.
                    full = nb < batch_size and b0 > 0 and not getattr(model, "training", True)
                    with torch.no_grad(), call_amp():
                        out = run(batch if full else batch[:nb])[:nb]      # inference.py:171-173
                    out = out.to(torch.float32).contiguous()
                    ctx.tile_accumulate(out, chunk, patch_size, trim, accum_pred, accum_wgt, shape)
                    if pbar is not None:
                        pbar.update(nb)
            del vol
            result = torch.empty(shape, dtype=torch.int16, device=dev)
            ctx.tile_finalize(transform.native_struct(), accum_pred, accum_wgt, result, n)
            stream.synchronize()
            out = result.cpu().numpy().view(np.uint16)
        finally:                                    # an exception must not leave the context on the caller's stream
            ctx.reset_stream()
            if pbar is not None:
                pbar.close()
    del run
    return out


def predict_store(src, dst_path, model, transform, batch_size=32, patch_size=64, overlap=12, trim=5,
                  verbose=True, fast=True, precision="fp32", codec=None, chunks=None, attributes=None,
                  budget_bytes=16 << 30, device=None, stats=None):
    """A stored volume in, the network's denoised and coded store out, without ever holding the volume: the result is
    ``write_zarr(predict(read_zarr(src)[0, 0], model, transform, ...), dst_path, ...)`` for a volume of any size
    (DESIGN.md 5.16).

    ``src``: a store's path or a ``StoredArray`` of uint16 (opened for the device used here).  The destination is
    made with ``chunk_store.create_zarr`` (``codec``: default ``ExacCodec(2)``; ``chunks``: default the source's;
    ``attributes``).  ``model``, ``transform``, ``batch_size``, ``patch_size``, ``overlap``, ``trim``, ``fast`` and
    ``precision`` mean what they mean in ``predict``.  ``device``: default the model's.

    The volume is cut into bricks of whole destination chunks that cost at most ``budget_bytes`` of device memory each
    (``utils.store_predict.plan_predict``; a single chunk is taken whatever it costs).  Per brick: the window its
    patches read comes from the source by a region read that stays on the device, every patch of ``predict``'s tiling
    whose core meets the brick is cut from it, transformed and run -- the same input values, zero padding included --
    and all predictions of the brick are stitched in one launch that adds them per voxel in ``predict``'s order (raster
    order of patch starts) and applies the same normalisation, inverse transform and rounding; the counts are
    scattered into a pool of destination chunks, coded and committed.  For a model whose output rows do not depend on
    the rest of the batch the store is therefore chunk file for chunk file what the whole-volume call gives.  Nothing
    is carried between bricks: a patch whose core meets several bricks runs once for each.

    ``transform`` is used as given: no per-volume offset is estimated, nothing here sees the whole volume.  Measure the
    store first -- ``m = utils.noise.measure_store(src)``, one pass out of core -- and pass
    ``build_volume_transform(base, img=m)``, which takes the offset the whole volume gives.

    Returns raw bytes / stored chunk bytes, like ``write_zarr``.  ``stats`` (a dict) receives ``seconds`` per phase
    (read, gather, forward, stitch, scatter, encode, files_write; the stream is synchronised around the phases, per
    batch for gather and forward, only when ``stats`` is given -- otherwise only a read, an encode or freeing a buffer
    waits for it), ``bricks``, ``patches_run``, ``patches_unique`` (``count_patches`` of
    the volume) and ``largest_alloc``, the most device bytes held here at one time (the model's activations are the
    framework's and are not counted)."""
    from aind_exaspim_image_compression.utils import chunk_store, store_predict, store_windows, store_write
    from aind_exaspim_image_compression.utils.chunk_codec import ExacCodec
    # -- every argument check, before a context exists
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, not {precision!r}")
    amp_dtype = PRECISIONS[precision]
    batch_size, patch_size, overlap, trim = int(batch_size), int(patch_size), int(overlap), int(trim)
    if batch_size < 1:
        raise ValueError("predict_store: batch_size >= 1")
    if patch_size < 1 or not overlap < patch_size:
        raise ValueError("predict_store: patch_size >= 1 and overlap < patch_size")
    if trim < 0 or patch_size - 2 * trim < 1:
        raise ValueError("predict_store: 0 <= trim and patch_size - 2 * trim >= 1")
    budget = int(budget_bytes)
    if budget < 1:
        raise ValueError("predict_store: budget_bytes must be positive")
    chunks = store_windows.check_chunks(chunks)
    # the device: the caller's, else the model's (no context is needed to tell); a path is opened for it
    dev = torch.device("cuda", int(device)) if device is not None else _model_device(model)
    index = dev.index or 0
    (arr,) = store_windows.open_u16_stores("predict_store", (("src", src),), index)
    shape = tuple(int(s) for s in arr.shape[2:])
    chunks = chunks if chunks is not None else tuple(int(c) for c in arr.chunks)
    codec = codec or ExacCodec(2)
    bricks = store_predict.plan_predict(shape, chunks[2:], patch_size, overlap, trim, batch_size, budget)
    most = max(b.n_patches for b in bricks)
    unique = count_patches(_ShapeOnly((1, 1) + shape), patch_size, overlap)

    _miopen_defaults()
    ctx = _native.context(index)
    out = chunk_store.create_zarr(dst_path, shape, chunks, codec=codec, attributes=attributes, overwrite=True,
                                  device=index)
    run, loop_amp, call_amp = _forward_plan(model, fast, amp_dtype)
    tf = transform.native_struct()
    pv = patch_size ** 3
    source = store_windows.StoreWindows([arr], chunks[2], fill=0)       # (in z slabs of a destination chunk)
    held = {"now": 0, "most": 0}

    def hold(nbytes):
        held["now"] += nbytes
        held["most"] = max(held["most"], held["now"])

    pbar = None
    if verbose:
        from tqdm import tqdm
        pbar = tqdm(total=sum(b.n_patches for b in bricks), desc="Denoise")
    patches_run, seen_batch = 0, False
    try:
        with torch.cuda.device(dev), store_windows.capped_pools([arr], budget):
            stream = torch.cuda.current_stream(dev)
            ctx.set_stream(stream.cuda_stream)       # kernels, the codecs and the model share one stream
            clock = store_windows.PhaseClock(
                ("read", "gather", "forward", "stitch", "scatter", "encode", "files_write"), stats is not None,
                stream.synchronize)
            seconds = clock.seconds
            # one input batch and one buffer of predictions, sized for the largest brick, for the whole call
            batch = torch.zeros((batch_size, 1, patch_size, patch_size, patch_size), dtype=torch.float32, device=dev)
            preds = torch.empty((max(most, 1), 1, patch_size, patch_size, patch_size), dtype=torch.float32,
                                device=dev)
            hold(4 * pv * (batch_size + max(most, 1)))
            with store_windows.BrickSink("predict_store", out, ctx, shape, chunks) as sink:
                for brick in bricks:
                    n_patches = brick.n_patches
                    grid = _native.patch_grid(brick.first, brick.count, patch_size - overlap, patch_size)
                    if n_patches:
                        t0 = time.perf_counter()
                        (d_win,), win_dims = source.read(brick.win_origin, brick.win_extent)
                        hold(2 * int(np.prod(win_dims)))
                        seconds["read"] += time.perf_counter() - t0
                        try:
                            with loop_amp():
                                for k0 in range(0, n_patches, batch_size):
                                    nb = min(batch_size, n_patches - k0)
                                    t0 = clock()
                                    ctx.tile_gather_u16(tf, d_win, brick.win_origin, win_dims, shape, grid, k0, nb,
                                                        batch)
                                    t1 = clock()
                                    # predict's rule for a short batch: at full size once the tensor holds earlier
                                    # rows (MIOpen sees ONE shape), for eval-mode modules only; the call's first batch
                                    # as it is
                                    full = nb < batch_size and seen_batch and not getattr(model, "training", True)
                                    with torch.no_grad(), call_amp():
                                        res = run(batch if full else batch[:nb])[:nb]
                                    preds[k0:k0 + nb].copy_(res)
                                    del res
                                    t2 = clock()
                                    seconds["gather"] += t1 - t0
                                    seconds["forward"] += t2 - t1
                                    seen_batch = True
                                    patches_run += nb
                                    if pbar is not None:
                                        pbar.update(nb)
                        finally:                                 # (freeing a buffer waits for the stream)
                            d_win.free()
                            hold(-2 * int(np.prod(win_dims)))
                    nvox = int(np.prod(brick.extent))
                    group = sink.pool([brick.origin], [brick.extent])
                    t0 = clock()
                    with ctx.alloc(2 * nvox) as d_res:
                        hold(2 * nvox)
                        ctx.tile_stitch_u16(tf, preds if n_patches else None, n_patches, grid, trim, brick.origin,
                                            brick.extent, shape, d_res)
                        t1 = clock()
                        with group as pool:
                            hold(2 * pool.g.pool_elems)
                            pool.scatter(d_res, nvox, np.uint16, store_write.box_records([brick.origin], brick.extent))
                            t2 = clock()
                            d_res.free()
                            hold(-2 * nvox)
                            seconds["stitch"] += t1 - t0
                            seconds["scatter"] += t2 - t1
                            pool.commit()
                        hold(-2 * pool.g.pool_elems)
            del batch, preds
    finally:
        ctx.reset_stream()
        if pbar is not None:
            pbar.close()
    del run
    if stats is not None:
        stats.update(sink.finish(seconds), seconds=seconds, bricks=len(bricks), patches_run=patches_run,
                     patches_unique=unique, largest_alloc=held["most"])
    return 2 * int(np.prod(shape)) / sink.written


def predict_patch(patch, model, transform):
    """Denoise one patch (reference inference.py:119-150); uint16, same shape as the input."""
    patch = np.asarray(patch)
    shape = patch.shape[-3:]
    x = transform.forward(patch.reshape(shape))
    dev = _model_device(model)
    with torch.no_grad():
        pred = model(to_tensor(x, device=dev))
    return transform.inverse(pred[0, 0].float().cpu().numpy())


# --- helpers (reference inference.py:178-252) -------------------------------------------------
class _ShapeOnly:
    def __init__(self, shape):
        self.shape = shape


def add_padding(patch, patch_size):
    """Zero-pad a 3-D patch at the high end of each axis up to ``patch_size`` (host helper kept
    for API parity; ``predict`` pads inside the gather kernel)."""
    patch = np.asarray(patch)
    pad = [(0, patch_size - s) for s in patch.shape]
    return np.pad(patch, pad, mode="constant", constant_values=0)


def generate_patch_starts(img, patch_size, overlap):
    """Patch corner coordinates: ``range(0, dim - patch + stride, stride)`` per spatial axis of
    a ``(1, 1, D, H, W)`` image, z outermost."""
    stride = patch_size - overlap
    axes = [range(0, img.shape[a] - patch_size + stride, stride) for a in (2, 3, 4)]
    return itertools.product(*axes)


def count_patches(img, patch_size, overlap):
    stride = patch_size - overlap
    n = 1
    for a in (2, 3, 4):
        n *= len(range(0, img.shape[a] - patch_size + stride, stride))
    return n


def load_model(path, device="cuda"):
    """Load a checkpoint -> ``(model.eval(), transform)`` (reference inference.py:255-299).

    Accepts the current format ``{"model", "model_config", "transform"}`` and a bare legacy
    ``state_dict`` (transform then defaults to asinh).  Unlike the reference, ``N2V2UNet``
    checkpoints work (the reference forgets to import the class: inference.py:290-291)."""
    _miopen_defaults()
    ckpt = torch.load(path, map_location=device)
    if isinstance(ckpt, dict) and "model" in ckpt:
        state_dict = ckpt["model"]
        transform_cfg = ckpt.get("transform") or {"kind": "asinh"}
        model_cfg = dict(ckpt.get("model_config") or {})
    else:
        state_dict, transform_cfg, model_cfg = ckpt, {"kind": "asinh"}, {}
    cls = N2V2UNet if model_cfg.pop("model", "UNet") == "N2V2UNet" else UNet
    model = cls(**model_cfg)
    model.load_state_dict(state_dict)
    model.to(device)
    model.eval()
    return model, build_transform(transform_cfg)


def build_volume_transform(base_transform, img=None, percentile=0.1, offset=None):
    """Inference transform carrying a per-volume background offset (reference
    inference.py:302-337): a supplied ``offset`` is used as is, otherwise it is estimated from
    ``img``; ``ValueError`` if neither is given.  ``img`` may be the ``StoreMeasure`` of a stored volume
    (``utils.noise.measure_store``), whose ``offset`` is the estimate of the whole volume."""
    if offset is None:
        if img is None:
            raise ValueError("img is required when offset is not supplied")
        from aind_exaspim_image_compression.utils.store_measure import StoreMeasure
        if isinstance(img, StoreMeasure):
            offset = img.offset(percentile=percentile, ignore_zeros=True)
        else:
            offset = estimate_offset(img, percentile=percentile, ignore_zeros=True)
    return with_offset(base_transform, offset)


def to_tensor(arr, device="cuda"):
    """numpy -> float tensor of shape (1, 1, D, H, W) on ``device`` (inference.py:340-359)."""
    arr = np.asarray(arr)
    while arr.ndim < 5:
        arr = arr[np.newaxis, ...]
    return torch.tensor(arr).to(device, dtype=torch.float)


def batch_to_tensor(arr, device="cuda"):
    """(B, D, H, W) numpy -> (B, 1, D, H, W) float tensor (inference.py:362-380)."""
    return to_tensor(np.asarray(arr)[:, np.newaxis, ...], device=device)
