"""Small seeded eval-mode fp32 models, built on the CPU, that ``predict``'s NDHWC shadow must handle beyond this
package's U-Nets (``inference._ndhwc_shadow`` / ``_fuse_norm_act``), each with what the rewrite should do to it.

A plain helper module (imported by ``test_shadow_rewrite.py`` and ``test_shadow_zoo_gpu.py``).  An ``Entry``:
    build()  -> the model (eval mode, fp32, CPU; GroupNorm gamma / beta set away from (1, 0))
    shape    the input's shape (N, C, D, H, W); the tests feed it as ``channels_last_3d``
    pairs    FusedGroupNormLeakyReLU modules in the shadow (GroupNorm + LeakyReLU pairs it replaces)
    inplace  how many of them overwrite their input (those right behind a Conv3d)
    biases   how many took over the bias of the convolution in front
    gn       of them, how many the kernels take (by channel count): native calls per forward on the GPU
    pool, up native max-pool / up-sampling modules, and native calls per forward on the GPU
Module counts are per slot of the module tree (``named_modules(remove_duplicate=False)``): every model here runs
each slot once per forward, so they are also the per-forward call counts.
    keep     names of modules whose outputs the model reads again later: a fused call must not change them
"""
import collections
import copy

import torch
from torch import nn

Entry = collections.namedtuple("Entry", "build shape pairs inplace biases gn pool up keep")


def _init(model, seed):
    """Seeded non-trivial parameters: GroupNorm gamma ~ N(1, 0.3), beta ~ N(0, 0.3); conv biases ~ N(0, 0.3)."""
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.GroupNorm) and m.affine:
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.Conv3d) and m.bias is not None:
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return model.eval()


def _seeded(cls, *args, seed=0, **kw):
    def build():
        torch.manual_seed(seed)
        return _init(cls(*copy.deepcopy(args), **copy.deepcopy(kw)), seed)     # (layers passed in: fresh ones)
    return build


class PreActResidual(nn.Module):
    """stem Conv3d(1 -> C), then ``h + Sequential(GN, LReLU, Conv3d, GN, LReLU, Conv3d)(h)``, a 1x1x1 head to one
    channel.  The first pair heads its container: its input ``h`` is read again by the residual sum."""

    def __init__(self, c=16, groups=4):
        super().__init__()
        self.stem = nn.Conv3d(1, c, 3, padding=1)
        self.body = nn.Sequential(nn.GroupNorm(groups, c), nn.LeakyReLU(0.01), nn.Conv3d(c, c, 3, padding=1),
                                  nn.GroupNorm(groups, c), nn.LeakyReLU(0.01), nn.Conv3d(c, c, 3, padding=1))
        self.head = nn.Conv3d(c, 1, 1)

    def forward(self, x):
        h = self.stem(x)
        return self.head(h + self.body(h))


class PassThroughPrefix(nn.Module):
    """``h + Sequential(prefix, GN, LReLU)(h)`` with a prefix that returns its own input (``Identity``, ``Dropout``
    in eval mode); ``h`` the output of a stem Conv3d(1 -> C), or the model's input itself (``stem=False``)."""

    def __init__(self, prefix, c=16, groups=4, stem=True):
        super().__init__()
        self.stem = nn.Conv3d(1, c, 3, padding=1) if stem else nn.Identity()
        self.block = nn.Sequential(prefix, nn.GroupNorm(groups, c), nn.LeakyReLU(0.2))

    def forward(self, x):
        h = self.stem(x)
        return h + self.block(h)


class SharedConv(nn.Module):
    """One Conv3d(cin -> cout) in ``Sequential(conv, GN, LReLU)`` and called directly as well:
    ``block(x) + conv(x)``, through an optional 1x1x1 head to one channel."""

    def __init__(self, cin, cout, groups, head=False):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 3, padding=1)
        self.block = nn.Sequential(self.conv, nn.GroupNorm(groups, cout), nn.LeakyReLU(0.01))
        self.head = nn.Conv3d(cout, 1, 1) if head else nn.Identity()

    def forward(self, x):
        return self.head(self.block(x) + self.conv(x))


class SharedBlock(nn.Module):
    """stem Conv3d(1 -> C), then one ``Sequential(Conv3d, GN, LReLU, MaxPool3d(2))`` held by two parents and run
    twice: its convolution sits in one slot of the tree (every call of it is followed by the fused pair), the
    block in two."""

    def __init__(self, c=8, groups=2):
        super().__init__()
        self.stem = nn.Conv3d(1, c, 3, padding=1)
        block = nn.Sequential(nn.Conv3d(c, c, 3, padding=1), nn.GroupNorm(groups, c), nn.LeakyReLU(0.01),
                              nn.MaxPool3d(2))
        self.first = block
        self.again = nn.ModuleList([block])

    def forward(self, x):
        return self.again[0](self.first(self.stem(x)))


def conv_norm_act(cin, c, groups, slope=0.01, affine=True, bias=True, act=None):
    """``Sequential(Conv3d(cin -> c), GroupNorm(groups, c), act)``, act LeakyReLU(slope) by default."""
    return nn.Sequential(nn.Conv3d(cin, c, 3, padding=1, bias=bias), nn.GroupNorm(groups, c, affine=affine),
                         act if act is not None else nn.LeakyReLU(slope))


def nested(cin, c, groups):
    """``Sequential(Conv3d, Sequential(GN, LReLU))``: the pair heads the inner container."""
    return nn.Sequential(nn.Conv3d(cin, c, 3, padding=1), nn.Sequential(nn.GroupNorm(groups, c), nn.LeakyReLU(0.01)))


def resample(cin, c, layer):
    """``Sequential(Conv3d(cin -> c), layer)``."""
    return nn.Sequential(nn.Conv3d(cin, c, 3, padding=1), layer)


class PoolUpSkip(nn.Module):
    """stem, then ``cat(h, up(pool(h)))`` and a 1x1x1 head: the skip reads ``h`` after the pool and up-sampling."""

    def __init__(self, c=8):
        super().__init__()
        self.stem = nn.Conv3d(1, c, 3, padding=1)
        self.pool = nn.MaxPool3d(2)
        self.up = nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True)
        self.head = nn.Conv3d(2 * c, 1, 1)

    def forward(self, x):
        h = self.stem(x)
        return self.head(torch.cat([h, self.up(self.pool(h))], dim=1))


def _up(**kw):
    return nn.Upsample(**{"scale_factor": 2, "mode": "trilinear", "align_corners": True, **kw})


ZOO = {
    # aliasing: a pair whose input is read again
    "preact_residual": Entry(_seeded(PreActResidual, seed=1), (3, 1, 12, 10, 16), 2, 1, 1, 2, 0, 0, ("stem",)),
    "preact_residual_b1": Entry(_seeded(PreActResidual, seed=2), (1, 1, 9, 14, 11), 2, 1, 1, 2, 0, 0, ("stem",)),
    "passthrough_identity": Entry(_seeded(PassThroughPrefix, nn.Identity(), seed=3), (3, 1, 12, 10, 16),
                                  1, 0, 0, 1, 0, 0, ("stem",)),
    "passthrough_dropout": Entry(_seeded(PassThroughPrefix, nn.Dropout(0.1), seed=4), (1, 1, 12, 10, 16),
                                 1, 0, 0, 1, 0, 0, ("stem",)),
    "passthrough_input": Entry(_seeded(PassThroughPrefix, nn.Identity(), stem=False, seed=5), (3, 16, 6, 5, 7),
                               1, 0, 0, 1, 0, 0, ()),
    # a convolution shared between a fused pair and a direct call keeps its bias
    "shared_conv_4_8": Entry(_seeded(SharedConv, 4, 8, 2, seed=6), (2, 4, 8, 8, 8), 1, 1, 0, 1, 0, 0, ()),
    "shared_conv_1_16": Entry(_seeded(SharedConv, 1, 16, 4, head=True, seed=7), (3, 1, 12, 10, 16),
                              1, 1, 0, 1, 0, 0, ()),
    "shared_conv_8_32": Entry(_seeded(SharedConv, 8, 32, 8, seed=8), (1, 8, 7, 6, 9), 1, 1, 0, 1, 0, 0, ()),
    # one block in two slots, run twice (counts are per slot, and per forward)
    "shared_block": Entry(_seeded(SharedBlock, seed=30), (2, 1, 16, 12, 20), 2, 2, 2, 2, 2, 0, ()),
    "conv_no_bias": Entry(_seeded(conv_norm_act, 4, 16, 4, bias=False, seed=9), (3, 4, 12, 10, 16),
                          1, 1, 0, 1, 0, 0, ()),
    "nested_sequential": Entry(_seeded(nested, 4, 16, 4, seed=10), (2, 4, 9, 8, 10), 1, 0, 0, 1, 0, 0, ()),
    # not fusable: must give the framework's result
    "gn_affine_false": Entry(_seeded(conv_norm_act, 4, 16, 4, affine=False, seed=11), (3, 4, 12, 10, 16),
                             0, 0, 0, 0, 0, 0, ()),
    "gn_relu": Entry(_seeded(conv_norm_act, 4, 16, 4, act=nn.ReLU(), seed=12), (1, 4, 12, 10, 16),
                     0, 0, 0, 0, 0, 0, ()),
    "gn_2_per_group": Entry(_seeded(conv_norm_act, 4, 16, 8, seed=13), (3, 4, 12, 10, 16), 1, 1, 1, 0, 0, 0, ()),
    "gn_3_12": Entry(_seeded(conv_norm_act, 4, 12, 3, seed=14), (2, 4, 7, 9, 8), 1, 1, 1, 0, 0, 0, ()),
    "gn_c2048": Entry(_seeded(conv_norm_act, 4, 2048, 32, seed=15), (1, 4, 3, 4, 5), 1, 1, 1, 0, 0, 0, ()),
    # at the kernels' channel limits: fused
    "gn_1_4_slope0": Entry(_seeded(conv_norm_act, 4, 4, 1, slope=0.0, seed=16), (3, 4, 12, 10, 16),
                           1, 1, 1, 1, 0, 0, ()),
    "gn_1_4_slope0.2": Entry(_seeded(conv_norm_act, 1, 4, 1, slope=0.2, seed=17), (1, 1, 9, 14, 11),
                             1, 1, 1, 1, 0, 0, ()),
    "gn_1_4_slope0.01": Entry(_seeded(conv_norm_act, 4, 4, 1, slope=0.01, seed=28), (2, 4, 5, 6, 7),
                              1, 1, 1, 1, 0, 0, ()),
    "gn_32_1024_slope0": Entry(_seeded(conv_norm_act, 4, 1024, 32, slope=0.0, seed=29), (2, 4, 2, 3, 2),
                               1, 1, 1, 1, 0, 0, ()),
    "gn_32_1024_slope0.01": Entry(_seeded(conv_norm_act, 4, 1024, 32, slope=0.01, seed=18), (3, 4, 3, 4, 5),
                                  1, 1, 1, 1, 0, 0, ()),
    "gn_32_1024_slope0.2": Entry(_seeded(conv_norm_act, 4, 1024, 32, slope=0.2, seed=19), (1, 4, 4, 2, 6),
                                 1, 1, 1, 1, 0, 0, ()),
    # resampling: native
    "maxpool_odd_5_7_9": Entry(_seeded(resample, 4, 8, nn.MaxPool3d(2), seed=20), (3, 4, 5, 7, 9),
                               0, 0, 0, 0, 1, 0, ()),
    "maxpool_tuple": Entry(_seeded(resample, 4, 8, nn.MaxPool3d((2, 2, 2)), seed=21), (1, 4, 12, 10, 16),
                           0, 0, 0, 0, 1, 0, ()),
    "upsample_tuple": Entry(_seeded(resample, 4, 8, _up(scale_factor=(2, 2, 2)), seed=22), (3, 4, 5, 3, 4),
                            0, 0, 0, 0, 0, 1, ()),
    "pool_up_skip": Entry(_seeded(PoolUpSkip, seed=23), (3, 1, 12, 10, 16), 0, 0, 0, 0, 1, 1, ("stem",)),
    # resampling: must fall back
    "maxpool_stride1": Entry(_seeded(resample, 4, 8, nn.MaxPool3d(2, stride=1), seed=24), (3, 4, 6, 5, 7),
                             0, 0, 0, 0, 0, 0, ()),
    "maxpool_ceil": Entry(_seeded(resample, 4, 8, nn.MaxPool3d(2, ceil_mode=True), seed=25), (1, 4, 5, 7, 9),
                          0, 0, 0, 0, 0, 0, ()),
    "upsample_align_false": Entry(_seeded(resample, 4, 8, _up(align_corners=False), seed=26), (3, 4, 5, 3, 4),
                                  0, 0, 0, 0, 0, 0, ()),
    "upsample_nearest": Entry(_seeded(resample, 4, 8, nn.Upsample(scale_factor=2, mode="nearest"), seed=27),
                              (1, 4, 5, 3, 4), 0, 0, 0, 0, 0, 0, ()),
}


def make_input(entry, seed=0):
    """The entry's input: N(0, 1) * 2 + 0.5, fp32, NCDHW on the CPU."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(entry.shape, generator=g) * 2 + 0.5
