"""Backbones behind the reference's plugin contract (models/build_models.py:25-29): a callable name that
returns an nn.Module exposing ``.channels`` and ``forward(x[B,3,H,W]) -> 4 NCHW feature maps``.

Internally every activation is a token-major ``[B*H*W, C]`` tensor in the compute dtype and every op is
a HIP kernel (segmentation_factory_amd.functional).  The NCHW maps handed to the head are zero-copy
permuted views of those token buffers.
"""

import torch
from torch import nn

from . import functional as Fh
from .containers import (BatchNormWeights, ChannelsFirstLayerNormWeights, ConvWeights, LayerNormWeights, LinearWeights,
                         _no_forward, init_mit_style)

# reference models/backbones/mit.py:149-156
mit_settings = {
    'B0': [[32, 64, 160, 256], [2, 2, 2, 2]],
    'B1': [[64, 128, 320, 512], [2, 2, 2, 2]],
    'B2': [[64, 128, 320, 512], [3, 4, 6, 3]],
    'B3': [[64, 128, 320, 512], [3, 4, 18, 3]],
    'B4': [[64, 128, 320, 512], [3, 8, 27, 3]],
    'B5': [[64, 128, 320, 512], [3, 6, 40, 3]],
}


class TokenMap:
    """A feature map as tokens: data [B*H*W, C] (+ geometry).  ``nchw()`` is the plugin-API view."""
    __slots__ = ('data', 'B', 'H', 'W')

    def __init__(self, data, B, H, W):
        self.data, self.B, self.H, self.W = data, B, H, W

    def nchw(self):
        return self.data.view(self.B, self.H, self.W, -1).permute(0, 3, 1, 2)


def tokens_from_nchw(x, dtype):
    """Accept an NCHW tensor from a foreign backbone/head: zero-copy when it is a permuted NHWC buffer."""
    B, C, H, W = x.shape
    t = x.permute(0, 2, 3, 1)
    if not t.is_contiguous() or t.dtype != dtype:
        from . import hip
        src = x.contiguous()
        t = hip.permute021(src, B, C, H * W, dtype)          # NCHW -> NHWC re-layout kernel
        return TokenMap(t.view(B * H * W, C), B, H, W)
    return TokenMap(t.reshape(B * H * W, C), B, H, W)


def _drop_path_scales(owner, rates, per_block, B, device):
    """Per block a tuple of `per_block` [B] rows of keep / kp scales (drop_path.py:18-25: x/kp*floor(kp+U)), all drawn as ONE
    [n_draws, B] tensor per forward; Nones outside training and for blocks with rate 0, which use nn.Identity in the reference and draw
    nothing.  owner.stochastic_override['drop_path'] (tests) replaces the draw with given keep flags [n_draws, B]."""
    if not owner.training or all(r == 0 for r in rates):
        return [(None,) * per_block] * len(rates)
    draws = [r for r in rates if r > 0 for _ in range(per_block)]
    if owner.stochastic_override is not None and 'drop_path' in owner.stochastic_override:
        kp = 1.0 - torch.tensor(draws, dtype=torch.float32, device=device)[:, None]
        scale = (owner.stochastic_override['drop_path'].to(device=device, dtype=torch.float32) / kp).contiguous()
    else:
        scale = Fh.stochastic_scales(owner, tuple(1.0 - r for r in draws), B, device)       # keep / kp, one row per draw
    out, i = [], 0
    for r in rates:
        out.append(tuple(scale[i + j] for j in range(per_block)) if r > 0 else (None,) * per_block)
        i += per_block if r > 0 else 0
    return out


class Attention(nn.Module):
    """Spatial-reduction attention (mit.py:9-59)."""

    def __init__(self, dim, head, sr_ratio):
        super().__init__()
        self.head, self.sr_ratio, self.dim = head, sr_ratio, dim
        self.q = LinearWeights(dim, dim)
        self.kv = LinearWeights(dim, dim * 2)
        self.proj = LinearWeights(dim, dim)
        if sr_ratio > 1:
            self.sr = ConvWeights(dim, dim, sr_ratio, sr_ratio)
            self.norm = LayerNormWeights(dim)
        self.apply(init_mit_style)

    def tokens(self, h, B, H, W, residual, rscale, col=None, q=None):
        N = H * W
        if col is not None:
            # the norm in front already wrote its output as the im2col matrix of the spatial-reduction convolution (layer_norm_res_patch):
            # no im2col / col2im passes, and the two consumers' gradients meet in the LayerNorm backward
            # (q given: the norm formed the q Linear's output as well -- layer_norm_res_patch_linear -- and h is None)
            sr = self.sr_ratio
            if q is None:
                q = Fh.linear(h, self.q.weight, self.q.bias)
            xr = Fh.conv_from_col(col, self.sr.weight, self.sr.bias, sr)
            xr = Fh.layer_norm(xr, self.norm.weight, self.norm.bias, self.norm.eps)
            Nkv = (H // sr) * (W // sr)
            kv = Fh.linear(xr, self.kv.weight, self.kv.bias)
            o = Fh.attention(q, kv, B, N, Nkv, self.head)
            return Fh.linear(o, self.proj.weight, self.proj.bias, residual=residual, rscale=rscale, rows_per_group=N)
        # two consumers (q and the key / value path): the key / value path's gradient joins inside q's data-gradient product
        q, h = Fh.linear_fork(h, self.q.weight, self.q.bias)
        if self.sr_ratio > 1:
            sr = self.sr_ratio
            xr = Fh.conv_patch(h, self.sr.weight, self.sr.bias, (B, H, W, self.dim, sr, sr, 0))
            xr = Fh.layer_norm(xr, self.norm.weight, self.norm.bias, self.norm.eps)
            Nkv = ((H - sr) // sr + 1) * ((W - sr) // sr + 1)
        else:
            xr, Nkv = h, N
        kv = Fh.linear(xr, self.kv.weight, self.kv.bias)
        o = Fh.attention(q, kv, B, N, Nkv, self.head)
        return Fh.linear(o, self.proj.weight, self.proj.bias, residual=residual, rscale=rscale, rows_per_group=N)


class DWConv(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dwconv = ConvWeights(dim, dim, 3, 1, 1, groups=dim)


class MLP(nn.Module):
    """fc1 -> depthwise 3x3 -> GELU -> fc2 (mit.py:74-99)."""

    def __init__(self, c1, c2):
        super().__init__()
        self.fc1 = LinearWeights(c1, c2)
        self.dwconv = DWConv(c2)
        self.fc2 = LinearWeights(c2, c1)
        self.apply(init_mit_style)

    def tokens(self, h, B, H, W, residual, rscale, hidden=False):
        f = h if hidden else Fh.linear(h, self.fc1.weight, self.fc1.bias)          # hidden: h is fc1's output already
        dw = self.dwconv.dwconv
        if Fh.dwconv3x3_gelu_linear_ok(f, self.fc2.weight, self.fc2.bias, dw.weight, dw.bias, B, H, W):
            # large maps: one formula for dwconv + GELU -> fc2, whose backward never stores fc2's hidden-width data gradient
            return Fh.dwconv3x3_gelu_linear(f, self.fc2.weight, self.fc2.bias, dw.weight, dw.bias, B, H, W, residual=residual, rscale=rscale)
        g = Fh.dwconv3x3_gelu(f, self.dwconv.dwconv.weight, self.dwconv.dwconv.bias, B, H, W, True)
        return Fh.linear(g, self.fc2.weight, self.fc2.bias, residual=residual, rscale=rscale, rows_per_group=H * W)


class PatchEmbed(nn.Module):
    """Overlapped patch embedding: strided conv + LayerNorm (mit.py:102-131)."""

    def __init__(self, c1=3, c2=32, patch_size=7, stride=4):
        super().__init__()
        self.c1, self.k, self.stride = c1, patch_size, stride
        self.proj = ConvWeights(c1, c2, patch_size, stride, patch_size // 2)
        self.norm = LayerNormWeights(c2)
        self.apply(init_mit_style)

    def tokens(self, x, B, H, W, image, dtype):
        k, s, p = self.k, self.stride, self.k // 2
        t = Fh.conv_patch(x, self.proj.weight, self.proj.bias, (B, H, W, self.c1, k, s, p), image=image, dtype=dtype)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        return Fh.layer_norm(t, self.norm.weight, self.norm.bias, self.norm.eps), Ho, Wo


class Block(nn.Module):
    """x + DropPath(Attn(LN(x)));  x + DropPath(MLP(LN(x)))   (mit.py:134-146).  The residual add and the
    per-sample DropPath scale are fused into the epilogue of the proj / fc2 GEMMs."""

    def __init__(self, dim, head, sr_ratio=1, dpr=0.):
        super().__init__()
        self.norm1 = LayerNormWeights(dim)
        self.attn = Attention(dim, head, sr_ratio)
        self.drop_prob = float(dpr)
        self.norm2 = LayerNormWeights(dim)
        self.mlp = MLP(dim, int(dim * 4))

    def tokens(self, x, B, H, W, scales):
        s1, s2 = scales
        sr = self.attn.sr_ratio
        if Fh.patch_layout_ok(W, H, sr) and x.is_cuda:
            qw = self.attn.q
            if Fh.layer_norm_res_patch_linear_ok(x, self.norm1.weight, self.norm1.bias, qw.weight, qw.bias):
                # stages 1 / 2 on large maps: norm1 -> q as one formula (the token-order LayerNorm output is never stored)
                x, q, col = Fh.layer_norm_res_patch_linear(x, self.norm1.weight, self.norm1.bias, self.norm1.eps, W, sr, qw.weight, qw.bias)
                x = self.attn.tokens(None, B, H, W, x, s1, col=col, q=q)
            else:
                x, h, col = Fh.layer_norm_res_patch(x, self.norm1.weight, self.norm1.bias, self.norm1.eps, W, sr)
                x = self.attn.tokens(h, B, H, W, x, s1, col=col)
        else:
            x, h = Fh.layer_norm_res(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)     # x passes through for the residual
            x = self.attn.tokens(h, B, H, W, x, s1)
        # norm2 -> mlp.fc1 as one formula where the fused backward exists (stages 1 / 2 on large maps), the two calls otherwise
        fc1 = self.mlp.fc1
        x, f = Fh.layer_norm_res_linear(x, self.norm2.weight, self.norm2.bias, self.norm2.eps, fc1.weight, fc1.bias)
        return self.mlp.tokens(f, B, H, W, x, s2, hidden=True)


class MiT(nn.Module):
    """Mix Transformer encoder (mit.py:159-218), variants B0-B5."""

    def __init__(self, model_name: str = 'B0', **kwargs):
        super().__init__()
        assert model_name in mit_settings.keys(), f"MiT model name should be in {list(mit_settings.keys())}"
        embed_dims, depths = mit_settings[model_name]
        drop_path_rate = 0.1
        self.channels = embed_dims
        self.depths = depths
        self.compute_dtype = torch.bfloat16
        self.stochastic_override = None      # tests: {'drop_path': keep[n_draws, B]}

        self.patch_embed1 = PatchEmbed(3, embed_dims[0], 7, 4)
        self.patch_embed2 = PatchEmbed(embed_dims[0], embed_dims[1], 3, 2)
        self.patch_embed3 = PatchEmbed(embed_dims[1], embed_dims[2], 3, 2)
        self.patch_embed4 = PatchEmbed(embed_dims[2], embed_dims[3], 3, 2)

        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        heads, srs = [1, 2, 5, 8], [8, 4, 2, 1]
        cur = 0
        for s in range(4):
            blocks = nn.ModuleList([Block(embed_dims[s], heads[s], srs[s], dpr[cur + i]) for i in range(depths[s])])
            setattr(self, f'block{s + 1}', blocks)
            setattr(self, f'norm{s + 1}', LayerNormWeights(embed_dims[s]))
            cur += depths[s]

    def _drop_path_scales(self, B, device):
        """One (attention, mlp) pair of [B] keep / kp scale rows per block"""
        return _drop_path_scales(self, [blk.drop_prob for s in range(4) for blk in getattr(self, f'block{s + 1}')], 2, B, device)

    def forward_tokens(self, x):
        """x: fp32 NCHW image.  Returns 4 TokenMaps (strides 4/8/16/32)."""
        B, _, H, W = x.shape
        dtype = self.compute_dtype
        scales = self._drop_path_scales(B, x.device)
        outs, bi = [], 0
        cur, image = x, True
        for s in range(4):
            pe = getattr(self, f'patch_embed{s + 1}')
            t, H, W = pe.tokens(cur, B, H, W, image, dtype)
            for blk in getattr(self, f'block{s + 1}'):
                t = blk.tokens(t, B, H, W, scales[bi])
                bi += 1
            nrm = getattr(self, f'norm{s + 1}')
            if s < 3:       # the stage output feeds the decode head AND the next patch embedding: one LayerNorm, two consumers
                t_head, t = Fh.layer_norm_fork(t, nrm.weight, nrm.bias, nrm.eps)
            else:
                t_head = t = Fh.layer_norm(t, nrm.weight, nrm.bias, nrm.eps)
            outs.append(TokenMap(t_head, B, H, W))
            cur, image = t, False
        return outs

    def forward(self, x):
        return tuple(tm.nchw() for tm in self.forward_tokens(x))


# ---- ConvNeXt / ConvNeXtV2 (models/backbones/convnext.py, convnextv2.py) -------------------------------------------------
# reference models/backbones/convnext.py:70-76
convnext_settings = {
    'T': [[3, 3, 9, 3], [96, 192, 384, 768], 0.1],
    'S': [[3, 3, 27, 3], [96, 192, 384, 768], 0.4],
    'B': [[3, 3, 27, 3], [128, 256, 512, 1024], 0.5],
    'L': [[3, 3, 27, 3], [192, 384, 768, 1536], 0.5],
    'XL': [[3, 3, 27, 3], [256, 512, 1024, 2048], 0.5],
}


def _init_convnext(m):
    """convnext.py:103-106 / convnextv2.py:164-167: trunc_normal(.02) weights, zero bias for Conv2d and Linear."""
    from .containers import trunc_normal_
    if isinstance(m, (nn.Conv2d, nn.Linear)):
        trunc_normal_(m.weight, std=.02)
        nn.init.constant_(m.bias, 0)


class GRNWeights(nn.Module):
    """Global Response Normalization parameters (convnextv2.py:68-80): gamma, beta of shape [1, 1, 1, dim]."""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.beta = nn.Parameter(torch.zeros(1, 1, 1, dim))


class ConvNeXtBlock(nn.Module):
    """dwconv 7x7 -> LayerNorm -> Linear 4x -> GELU -> [GRN] -> Linear -> [x gamma] -> DropPath + residual
    (convnext.py:26-51; convnextv2.py:83-113).  The layer scale is folded into pwconv2's parameters and the residual +
    per-sample DropPath scale into its GEMM epilogue."""

    def __init__(self, dim, dpr=0., init_value=1e-6, v2=False):
        super().__init__()
        self.dim, self.v2 = dim, v2
        self.dwconv = ConvWeights(dim, dim, 7, 1, 3, groups=dim)
        self.norm = LayerNormWeights(dim, eps=1e-6)
        self.pwconv1 = LinearWeights(dim, 4 * dim)
        if v2:
            self.grn = GRNWeights(4 * dim)           # registered between the linears, as in convnextv2.py:92-94 (state_dict order)
        self.pwconv2 = LinearWeights(4 * dim, dim)
        if v2:
            pass
        elif init_value > 0:
            self.gamma = nn.Parameter(init_value * torch.ones((dim)), requires_grad=True)
        self.drop_prob = float(dpr)
        self.fp8 = False          # forward products of pwconv1 / pwconv2 on the fp8 matrix pipe (SegmentationModel.set_fp8)

    def tokens(self, x, B, H, W, scale):
        x, xc = Fh.fork(x, 2)                        # residual + depthwise conv both read x
        h = Fh.dwconv7x7(xc, self.dwconv.weight, self.dwconv.bias, B, H, W)
        h = Fh.layer_norm(h, self.norm.weight, self.norm.bias, self.norm.eps)
        h = Fh.linear(h, self.pwconv1.weight, self.pwconv1.bias, fp8=self.fp8)
        if self.v2:
            # act -> grn (convnextv2.py:92-94) as one op: the GELU is applied inside the GRN kernels, gelu(h) is never written
            if Fh.hip.policy('no_gelu_grn'):
                h = Fh.grn(Fh.gelu(h), self.grn.gamma, self.grn.beta, B, H * W)
            else:
                h = Fh.grn(h, self.grn.gamma, self.grn.beta, B, H * W, pre_gelu=True)
            return Fh.linear(h, self.pwconv2.weight, self.pwconv2.bias, residual=x, rscale=scale, rows_per_group=H * W, fp8=self.fp8)
        h = Fh.gelu(h)
        if hasattr(self, 'gamma'):
            return Fh.linear_layer_scale(h, self.pwconv2.weight, self.pwconv2.bias, self.gamma, residual=x, rscale=scale,
                                         rows_per_group=H * W)
        return Fh.linear(h, self.pwconv2.weight, self.pwconv2.bias, residual=x, rscale=scale, rows_per_group=H * W)


class _ConvNeXtBase(nn.Module):
    """Shared trunk of ConvNeXt (convnext.py:79-120) and ConvNeXtV2 (convnextv2.py:116-178): stem conv k4 s4 + channels-first
    LayerNorm, three [LayerNorm + conv k2 s2] downsamplers, four block stages, one output LayerNorm per stage.  The
    channels-first LayerNorm of the reference is the ordinary row LayerNorm on NHWC tokens (eps 1e-6, biased variance)."""

    def _build(self, depths, dims, drop_path_rate, v2):
        self.channels = dims
        self.depths = depths
        self.compute_dtype = torch.bfloat16
        self.stochastic_override = None      # tests: {'drop_path': keep[n_draws, B]}
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(ConvWeights(3, dims[0], 4, 4), ChannelsFirstLayerNormWeights(dims[0])))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(ChannelsFirstLayerNormWeights(dims[i]), ConvWeights(dims[i], dims[i + 1], 2, 2)))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.stages = nn.ModuleList()
        cur = 0
        for i in range(4):
            self.stages.append(nn.Sequential(*[ConvNeXtBlock(dims[i], dpr[cur + j], v2=v2) for j in range(depths[i])]))
            cur += depths[i]
        for i in range(4):
            self.add_module(f'norm{i}', ChannelsFirstLayerNormWeights(dims[i]))
        self.apply(_init_convnext)

    def _drop_path_scales(self, B, device):
        """One [B] keep / kp scale row per block"""
        return [s for s, in _drop_path_scales(self, [blk.drop_prob for st in self.stages for blk in st], 1, B, device)]

    def forward_tokens(self, x):
        B, _, H, W = x.shape
        dtype = self.compute_dtype
        scales = self._drop_path_scales(B, x.device)
        outs, bi = [], 0
        t = None
        for i in range(4):
            ds = self.downsample_layers[i]
            if i == 0:
                conv, ln = ds[0], ds[1]
                t = Fh.conv_patch(x, conv.weight, conv.bias, (B, H, W, 3, 4, 4, 0), image=True, dtype=dtype)
                H, W = (H - 4) // 4 + 1, (W - 4) // 4 + 1
                t = Fh.layer_norm(t, ln.weight, ln.bias, ln.eps)
            else:
                ln, conv = ds[0], ds[1]
                t = Fh.layer_norm(t, ln.weight, ln.bias, ln.eps)
                t = Fh.conv_patch(t, conv.weight, conv.bias, (B, H, W, self.channels[i - 1], 2, 2, 0))
                H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
            for blk in self.stages[i]:
                t = blk.tokens(t, B, H, W, scales[bi])
                bi += 1
            nrm = getattr(self, f'norm{i}')
            if i < 3:
                t, th = Fh.fork(t, 2)                # the stage output feeds its output norm and the next downsampler's norm
            else:
                th = t
            outs.append(TokenMap(Fh.layer_norm(th, nrm.weight, nrm.bias, nrm.eps), B, H, W))
        return outs

    def forward(self, x):
        return [tm.nchw() for tm in self.forward_tokens(x)]


class ConvNeXt(_ConvNeXtBase):
    """models/backbones/convnext.py:79-120; the reference's plugin API only reaches the default variant 'T'."""

    def __init__(self, model_name: str = 'T') -> None:
        super().__init__()
        assert model_name in convnext_settings.keys(), f"ConvNeXt model name should be in {list(convnext_settings.keys())}"
        depths, embed_dims, drop_path_rate = convnext_settings[model_name]
        self._build(depths, embed_dims, drop_path_rate, v2=False)


class ConvNeXtV2(_ConvNeXtBase):
    """models/backbones/convnextv2.py:116-178 (GRN blocks, no layer scale)."""

    def __init__(self, in_chans=3, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), drop_path_rate=0.):
        super().__init__()
        assert in_chans == 3
        self._build(list(depths), list(dims), drop_path_rate, v2=True)


# factory functions with the reference's names (incl. its 'convnext_pico' spelling), widths and stochastic-depth rates
# (convnextv2.py:181-233)
def convnextv2_atto(**kw):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[40, 80, 160, 320], drop_path_rate=0.0, **kw)


def convnextv2_femto(**kw):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[48, 96, 192, 384], drop_path_rate=0.0, **kw)


def convnext_pico(**kw):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[64, 128, 256, 512], drop_path_rate=0.0, **kw)


def convnextv2_nano(**kw):
    return ConvNeXtV2(depths=[2, 2, 8, 2], dims=[80, 160, 320, 640], drop_path_rate=0.0, **kw)


def convnextv2_tiny(**kw):
    return ConvNeXtV2(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.1, **kw)


def convnextv2_base(**kw):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024], drop_path_rate=0.4, **kw)


def convnextv2_large(**kw):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[192, 384, 768, 1536], drop_path_rate=0.5, **kw)


def convnextv2_huge(**kw):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[352, 704, 1408, 2816], drop_path_rate=0.5, **kw)


def layer_id_map(backbone):
    """{parameter name (as in backbone.named_parameters()): layer id} for layer-wise learning-rate decay (optim.param_groups_lr_scale,
    --layer-decay).  Id 0 is the stem (MiT's patch_embed1, ConvNeXt's downsample_layers.0); the blocks count from 1 in forward order
    through the four stages; a stage's patch embedding / downsample layer takes the id of the first block it feeds; a stage-closing
    normN takes the id of the stage's last block.  Whoever consumes the map puts the decode head at max(ids) + 1.  Built for the
    families of the BASELINE configurations: MiT, ConvNeXt, ConvNeXtV2."""
    if isinstance(backbone, MiT):
        embed = lambda s: f'patch_embed{s + 1}.'
        block = lambda s, j: f'block{s + 1}.{j}.'
        norm = lambda s: f'norm{s + 1}.'
    elif isinstance(backbone, _ConvNeXtBase):
        embed = lambda s: f'downsample_layers.{s}.'
        block = lambda s, j: f'stages.{s}.{j}.'
        norm = lambda s: f'norm{s}.'
    else:
        raise ValueError(f'layer_id_map: no layer ids for the {type(backbone).__name__} family (built for MiT, ConvNeXt, ConvNeXtV2)')
    prefix, first = {}, 1
    for s, depth in enumerate(backbone.depths):
        prefix[embed(s)] = 0 if s == 0 else first
        for j in range(depth):
            prefix[block(s, j)] = first + j
        prefix[norm(s)] = first + depth - 1
        first += depth
    ids = {}
    for name, _ in backbone.named_parameters():
        hit = [i for p, i in prefix.items() if name.startswith(p)]
        if len(hit) != 1:
            raise ValueError(f'layer_id_map: parameter {name!r} of {type(backbone).__name__} belongs to no layer')
        ids[name] = hit[0]
    return ids


# ---- MobileNetV2 (models/backbones/mobilenetv2.py) ------------------------------------------------------------------------
def _bn_act(x, bn, training, act):
    """BatchNorm2d (+ReLU6) of mobilenetv2.ConvModule (mobilenetv2.py:5-11) / the bare BatchNorm2d of :29."""
    y = Fh.batch_norm_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps, act=act)
    if training:
        Fh.hip.add_i64_(bn.num_batches_tracked, 1)
    return y


class MBConvModule(nn.Sequential):
    """Conv2d(bias=False) + BatchNorm2d + ReLU6 with the reference's keys `<name>.0.weight`, `<name>.1.*`
    (mobilenetv2.py:5-11; the ReLU6 at index 2 has no parameters)."""

    def __init__(self, c1, c2, k, s=1, p=0, g=1):
        super().__init__(ConvWeights(c1, c2, k, s, p, 1, g, bias=False), BatchNormWeights(c2))
        self.k, self.s, self.g = k, s, g


class InvertedResidual(nn.Module):
    """mobilenetv2.py:14-37: [1x1 expand + BN + ReLU6] -> 3x3 depthwise (stride s) + BN + ReLU6 -> 1x1 project + BN
    (+ residual when s == 1 and c1 == c2)."""

    def __init__(self, c1, c2, s, expand_ratio):
        super().__init__()
        ch = int(round(c1 * expand_ratio))
        self.use_res_connect = s == 1 and c1 == c2
        self.stride, self.ch, self.expand = s, ch, expand_ratio != 1
        layers = []
        if self.expand:
            layers.append(MBConvModule(c1, ch, 1))
        layers.extend([MBConvModule(ch, ch, 3, s, 1, g=ch), ConvWeights(ch, c2, 1, bias=False), BatchNormWeights(c2)])
        self.conv = nn.Sequential(*layers)

    def tokens(self, x, B, H, W, training):
        if self.use_res_connect:
            x, h = Fh.fork(x, 2)
        else:
            h = x
        li = 0
        if self.expand:
            m = self.conv[li]
            h = _bn_act(Fh.linear(h, m[0].weight), m[1], training, 2)
            li += 1
        m = self.conv[li]
        h = Fh.dwconv3x3_gelu(h, m[0].weight, None, B, H, W, False)           # depthwise 3x3, pad 1, no bias, no GELU
        if self.stride > 1:
            h = Fh.subsample(h, B, H, W, self.stride)
            H, W = (H - 1) // self.stride + 1, (W - 1) // self.stride + 1
        h = _bn_act(h, m[1], training, 2)
        h = _bn_act(Fh.linear(h, self.conv[li + 1].weight), self.conv[li + 2], training, 0)
        return (Fh.add(x, h) if self.use_res_connect else h), H, W


class MobileNetV2(nn.Module):
    """models/backbones/mobilenetv2.py:45-92 (width 1.0): Conv-BN-ReLU6 stem + 17 inverted residuals, feature taps after
    features 3, 6, 13, 17 -> channels [24, 32, 96, 320] at strides 4 / 8 / 16 / 32."""

    def __init__(self, variant: str = None):
        super().__init__()
        self.out_indices = [3, 6, 13, 17]
        self.channels = [24, 32, 96, 320]
        self.compute_dtype = torch.bfloat16
        input_channel = 32
        setting = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]]   # t, c, n, s
        self.features = nn.ModuleList([MBConvModule(3, input_channel, 3, 2, 1)])
        for t, c, n, s in setting:
            for i in range(n):
                self.features.append(InvertedResidual(input_channel, c, s if i == 0 else 1, t))
                input_channel = c
        for m in self.modules():                                # mobilenetv2.py:68-79
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward_tokens(self, x):
        B, _, H, W = x.shape
        tr = self.training
        stem = self.features[0]
        t = Fh.conv_patch(x, stem[0].weight, None, (B, H, W, 3, 3, 2, 1), image=True, dtype=self.compute_dtype)
        H, W = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        t = _bn_act(t, stem[1], tr, 2)
        outs = []
        for i in range(1, len(self.features)):
            t, H, W = self.features[i].tokens(t, B, H, W, tr)
            if i in self.out_indices:
                if i != len(self.features) - 1:
                    t, th = Fh.fork(t, 2)            # feature tap: decode head + the next inverted residual
                else:
                    th = t
                outs.append(TokenMap(th, B, H, W))
        return outs

    def forward(self, x):
        return [tm.nchw() for tm in self.forward_tokens(x)]


# ---- CrossFormer (models/backbones/crossformer.py) -------------------------------------------------------------------------
def _small_linear(x, w, b):
    """x [T, K] W^T + b for the position-bias MLP (K <= 64, T = (2G-1)^2 rows): a broadcast multiply and a reduction, fp32."""
    return (x.unsqueeze(1) * w.unsqueeze(0)).sum(-1) + b


class _BiasGatherFn(torch.autograd.Function):
    """relative_position_bias = pos[relative_position_index] as [heads, N, N] (crossformer.py:148-150).  The backward sums the
    gradient per table row through a precomputed list of the (i, j) pairs that read the row: a gather and a reduction in a fixed
    order, where index_select's own backward would add with floating-point atomics."""

    @staticmethod
    def forward(ctx, pos, idx, pairs, N):
        ctx.save_for_backward(pairs)
        ctx.N = N
        return pos.t()[:, idx].reshape(pos.shape[1], N, N).contiguous()

    @staticmethod
    def backward(ctx, d):
        pairs, = ctx.saved_tensors
        heads, N = d.shape[0], ctx.N
        dflat = torch.cat([d.reshape(heads, N * N), d.new_zeros(heads, 1)], 1)          # slot N*N: the zero the short rows point at
        return dflat[:, pairs.reshape(-1)].reshape(heads, pairs.shape[0], pairs.shape[1]).sum(-1).t(), None, None, None


class _PosNorm(nn.Sequential):
    """LayerNorm -> ReLU -> Linear with the reference's keys `.0.*` / `.2.*` (crossformer.py:48-62)."""

    def __init__(self, dim, out):
        super().__init__(LayerNormWeights(dim), nn.Identity(), LinearWeights(dim, out))


class DynamicPosBias(nn.Module):
    """crossformer.py:36-72 with residual=False: an MLP from the (dh, dw) offset to one bias per head.  The table has (2G-1)^2 rows (169
    for G = 7) of pos_dim <= 64 channels: it is computed once per forward per block with torch ops in fp32 on the current stream (off the
    hot path; captured into the step's graph like everything else), and autograd carries the attention kernel's dbias back to pos.*."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.pos_dim = dim // 4
        self.pos_proj = LinearWeights(2, self.pos_dim)
        self.pos1 = _PosNorm(self.pos_dim, self.pos_dim)
        self.pos2 = _PosNorm(self.pos_dim, self.pos_dim)
        self.pos3 = _PosNorm(self.pos_dim, self.num_heads)
        self._tables = {}

    def tables(self, G, device):
        """(offsets [T, 2] fp32, relative_position_index [N*N], per-row reader lists [T, N]) of a G x G group (crossformer.py:129-144)."""
        key = (G, str(device))
        if key not in self._tables:
            rng = torch.arange(1 - G, G)
            offsets = torch.stack(torch.meshgrid([rng, rng], indexing='ij')).flatten(1).t().contiguous().float()
            co = torch.stack(torch.meshgrid([torch.arange(G), torch.arange(G)], indexing='ij')).flatten(1)
            rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
            idx = ((rel[:, :, 0] + G - 1) * (2 * G - 1) + rel[:, :, 1] + G - 1).reshape(-1)
            N, T = G * G, (2 * G - 1) ** 2
            pairs = torch.full((T, N), N * N, dtype=torch.int64)
            fill = [0] * T
            for flat, t in enumerate(idx.tolist()):
                pairs[t, fill[t]] = flat
                fill[t] += 1
            self._tables[key] = tuple(t.to(device) for t in (offsets, idx, pairs))
        return self._tables[key]

    def bias(self, G, device):
        """[heads, G*G, G*G] fp32"""
        offsets, idx, pairs = self.tables(G, device)
        pos = _small_linear(offsets, self.pos_proj.weight, self.pos_proj.bias)
        for m in (self.pos1, self.pos2, self.pos3):
            pos = torch.relu(torch.nn.functional.layer_norm(pos, (self.pos_dim,), m[0].weight, m[0].bias, m[0].eps))
            pos = _small_linear(pos, m[2].weight, m[2].bias)
        return _BiasGatherFn.apply(pos, idx, pairs, G * G)


class CrossFormerAttention(nn.Module):
    """crossformer.py:82-110: parameters of the grouped attention; head dim 32 in all four variants."""

    def __init__(self, dim, num_heads):
        super().__init__()
        assert dim == 32 * num_heads
        self.dim, self.num_heads = dim, num_heads
        # (quirk, :103) built as DynamicPosBias(dim // 4, ...): the module divides by 4 again, so pos_dim is dim // 16
        self.pos = DynamicPosBias(dim // 4, num_heads)
        self.qkv = LinearWeights(dim, dim * 3)
        self.proj = LinearWeights(dim, dim)


class CrossFormerMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = LinearWeights(dim, hidden)
        self.fc2 = LinearWeights(hidden, dim)


class CrossFormerBlock(nn.Module):
    """x + DropPath(GroupAttn(LN(x)));  x + DropPath(MLP(LN(x)))   (crossformer.py:191-352; use_acl / use_cpe off)."""

    def __init__(self, dim, num_heads, group_size=7, interval=8, lsda_flag=0, dpr=0.):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.group_size, self.interval, self.lsda_flag = group_size, interval, lsda_flag
        self.norm1 = LayerNormWeights(dim)
        self.attn = CrossFormerAttention(dim, num_heads)
        self.drop_prob = float(dpr)
        self.norm2 = LayerNormWeights(dim)
        self.mlp = CrossFormerMlp(dim, int(dim * 4))

    def grouping(self, H, W):
        """(group side, interval, lda) for an H x W map.  (quirk, :263-269) when min(H, W) <= group_size the block uses ONE group of side
        max(H, W) and sets its own lsda_flag to 0 for good: module state mutated in forward, so an LDA block that has once seen a small
        map stays in SDA mode.  Padding (:282-285) is to interval * G in LDA mode, to G in SDA mode, right and bottom only: the kernel's."""
        if min(H, W) <= self.group_size:
            self.lsda_flag = 0
            G = max(H, W)
        else:
            G = self.group_size
        return G, self.interval, self.lsda_flag == 1

    def tokens(self, x, B, H, W, scales):
        s1, s2 = scales
        G, interval, lda = self.grouping(H, W)
        x, h = Fh.layer_norm_res(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        qkv = Fh.linear(h, self.attn.qkv.weight, self.attn.qkv.bias)
        bias = self.attn.pos.bias(G, x.device)
        o = Fh.group_attention(qkv, bias, B, H, W, self.num_heads, G, interval, lda)
        x = Fh.linear(o, self.attn.proj.weight, self.attn.proj.bias, residual=x, rscale=s1, rows_per_group=H * W)
        x, h = Fh.layer_norm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        f = Fh.gelu(Fh.linear(h, self.mlp.fc1.weight, self.mlp.fc1.bias))
        return Fh.linear(f, self.mlp.fc2.weight, self.mlp.fc2.bias, residual=x, rscale=s2, rows_per_group=H * W)


class CrossFormerPatchEmbed(nn.Module):
    """crossformer.py:532-582 with patch_size=[4]: one conv k4 s4 p0 + LayerNorm."""

    def __init__(self, embed_dim):
        super().__init__()
        self.projs = nn.ModuleList([ConvWeights(3, embed_dim, 4, 4, 0)])
        self.norm = LayerNormWeights(embed_dim)


class CrossFormerPatchMerging(nn.Module):
    """crossformer.py:380-423 with patch_size=[2]: LayerNorm + one conv k2 s2 p0 to twice the width."""

    def __init__(self, dim):
        super().__init__()
        self.reductions = nn.ModuleList([ConvWeights(dim, 2 * dim, 2, 2, 0)])
        self.norm = LayerNormWeights(dim)


class CrossFormerStage(nn.Module):
    def __init__(self, dim, depth, num_heads, group_size, interval, dprs, downsample):
        super().__init__()
        # even blocks SDA, odd blocks LDA (:475)
        self.blocks = nn.ModuleList([CrossFormerBlock(dim, num_heads, group_size, interval, i % 2, dprs[i]) for i in range(depth)])
        self.downsample = CrossFormerPatchMerging(dim) if downsample else None


class CrossFormer(nn.Module):
    """models/backbones/crossformer.py:598-782 as its four factories build it: patch_size [4], merge_size [[2], [2], [2]], group size 7,
    intervals [8, 4, 2, 1], mlp ratio 4, drop-path rates linspace(0, 0.1, sum(depths)); ape, use_cpe and use_acl off.  The stage outputs
    go to the decode head as they are (no output norm)."""

    def __init__(self, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), group_size=(7, 7, 7, 7), crs_interval=(8, 4, 2, 1),
                 drop_path_rate=0.1):
        super().__init__()
        self.channels = [embed_dim, embed_dim * 2, embed_dim * 4, embed_dim * 8]
        self.depths = list(depths)
        self.compute_dtype = torch.bfloat16
        self.stochastic_override = None      # tests: {'drop_path': keep[n_draws, B]}
        self.patch_embed = CrossFormerPatchEmbed(embed_dim)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i in range(4):
            self.layers.append(CrossFormerStage(embed_dim * 2 ** i, depths[i], num_heads[i], group_size[i], crs_interval[i],
                                                dpr[sum(depths[:i]):sum(depths[:i + 1])], i < 3))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        """crossformer.py:749-758: trunc_normal(.02) on Linear weights, LayerNorm at 1 / 0; Linear biases and the Conv2d weights of
        patch_embed.projs / downsample.reductions keep torch's default initialisation."""
        from .containers import trunc_normal_
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _blocks(self):
        return [blk for st in self.layers for blk in st.blocks]

    def _drop_path_scales(self, B, device):
        """One (attention, mlp) pair of [B] keep / kp scale rows per block: the block's one DropPath module is applied twice (:342-343)"""
        return _drop_path_scales(self, [blk.drop_prob for blk in self._blocks()], 2, B, device)

    def forward_tokens(self, x):
        """x: fp32 NCHW image.  Returns 4 TokenMaps (strides 4/8/16/32)."""
        B, _, H, W = x.shape
        dtype = self.compute_dtype
        scales = self._drop_path_scales(B, x.device)
        pe = self.patch_embed
        t = Fh.conv_patch(x, pe.projs[0].weight, pe.projs[0].bias, (B, H, W, 3, 4, 4, 0), image=True, dtype=dtype)
        H, W = (H - 4) // 4 + 1, (W - 4) // 4 + 1
        t = Fh.layer_norm(t, pe.norm.weight, pe.norm.bias, pe.norm.eps)
        outs, bi = [], 0
        for i, st in enumerate(self.layers):
            for blk in st.blocks:
                t = blk.tokens(t, B, H, W, scales[bi])
                bi += 1
            if st.downsample is None:
                outs.append(TokenMap(t, B, H, W))
                break
            t, th = Fh.fork(t, 2)                    # the stage output feeds the decode head and the patch merging
            outs.append(TokenMap(th, B, H, W))
            ds = st.downsample
            assert H % 2 == 0 and W % 2 == 0, f"x size ({H}*{W}) are not even."
            t = Fh.layer_norm(t, ds.norm.weight, ds.norm.bias, ds.norm.eps)
            t = Fh.conv_patch(t, ds.reductions[0].weight, ds.reductions[0].bias, (B, H, W, self.channels[i], 2, 2, 0))
            H, W = H // 2, W // 2
        return outs

    def forward(self, x):
        return [tm.nchw() for tm in self.forward_tokens(x)]


# the reference's factories (crossformer.py:785-825)
def crossformer_tiny(**kw):
    return CrossFormer(embed_dim=64, depths=[1, 1, 8, 6], num_heads=[2, 4, 8, 16], **kw)


def crossformer_small(**kw):
    return CrossFormer(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], **kw)


def crossformer_base(**kw):
    return CrossFormer(embed_dim=96, depths=[2, 2, 18, 2], num_heads=[3, 6, 12, 24], **kw)


def crossformer_large(**kw):
    return CrossFormer(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], **kw)


# ---- CAS-ViT / RCViT (models/backbones/casvit.py) -------------------------------------------------------------------------------
class _SpatialOperation(nn.Module):
    """casvit.py:68-80: x * sigmoid(conv1x1_to_1(ReLU(BN(dw3x3(x))))); keys block.{0,1,3}.* (ReLU at 2, Sigmoid at 4)."""

    def __init__(self, dim):
        super().__init__()
        self.block = nn.Sequential(ConvWeights(dim, dim, 3, 1, 1, groups=dim), BatchNormWeights(dim), nn.Identity(),
                                   ConvWeights(dim, 1, 1, 1, 0, bias=False), nn.Identity())


class _ChannelOperation(nn.Module):
    """casvit.py:82-92: x * sigmoid(Wc mean_pixels(x)); key block.1.weight (the pool at 0, Sigmoid at 2)."""

    def __init__(self, dim):
        super().__init__()
        self.block = nn.Sequential(nn.Identity(), ConvWeights(dim, dim, 1, 1, 0, bias=False), nn.Identity())


class _LocalIntegration(nn.Module):
    """casvit.py:94-109 as Stage builds it: conv1x1 -> BatchNorm -> depthwise 3x3 -> GELU -> conv1x1; keys network.{0,1,2,4}.*."""

    def __init__(self, dim):
        super().__init__()
        self.network = nn.Sequential(ConvWeights(dim, dim, 1, 1, 0), BatchNormWeights(dim), ConvWeights(dim, dim, 3, 1, 1, groups=dim),
                                     nn.Identity(), ConvWeights(dim, dim, 1, 1, 0))


class AdditiveTokenMixer(nn.Module):
    """casvit.py:112-138: proj(dwc(ChannelOp(SpatialOp(q)) + ChannelOp(SpatialOp(k))) * v), q, k, v = chunk3(conv1x1(x))."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.qkv = ConvWeights(dim, 3 * dim, 1, 1, 0, bias=False)
        self.oper_q = nn.Sequential(_SpatialOperation(dim), _ChannelOperation(dim))
        self.oper_k = nn.Sequential(_SpatialOperation(dim), _ChannelOperation(dim))
        self.dwc = ConvWeights(dim, dim, 3, 1, 1, groups=dim)
        self.proj = ConvWeights(dim, dim, 3, 1, 1, groups=dim)

    @staticmethod
    def _gated(oper, t, B, H, W, training):
        """(SpatialOp(t), ChannelOp's gate [B, C] fp32).  t feeds the gate's depthwise conv and the gated product: a fork."""
        sp, ch = oper[0].block, oper[1].block
        ta, tb = Fh.fork(t, 2)
        r = Fh.dwconv3x3_gelu(ta, sp[0].weight, sp[0].bias, B, H, W, False)
        r = _bn_act(r, sp[1], training, 1)
        y, pool = Fh.spatial_gate(tb, r, sp[3].weight, B, H * W)
        # the channel gate: a [B, C] x [C, C] product per operator, fp32 torch ops on the current stream (off the hot path, captured into
        # the step's graph like DynamicPosBias.bias); autograd carries the kernels' gate gradients back to the weight and to `pool`
        C = pool.shape[1]
        gate = torch.sigmoid(((pool * (1.0 / (H * W))).unsqueeze(1) * ch[1].weight.view(C, C).unsqueeze(0)).sum(-1))
        return y, gate

    def tokens(self, x, B, H, W, training):
        q, k, v = Fh.qkv_split3(x, self.qkv.weight)
        q1, gq = self._gated(self.oper_q, q, B, H, W, training)
        k1, gk = self._gated(self.oper_k, k, B, H, W, training)
        u = Fh.channel_gate_mix(q1, k1, gq, gk, B, H * W)
        a = Fh.dwconv3x3_gelu(u, self.dwc.weight, self.dwc.bias, B, H, W, False)
        z = Fh.gated_mul(a, v)
        return Fh.dwconv3x3_gelu(z, self.proj.weight, self.proj.bias, B, H, W, False)


class _RCViTMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = ConvWeights(dim, hidden, 1)
        self.fc2 = ConvWeights(hidden, dim, 1)


class AdditiveBlock(nn.Module):
    """casvit.py:142-162 as Stage builds it (norm_layer = BatchNorm2d, act_layer = GELU, drop = drop_path = 0: no stochastic module):
    x + LocalIntegration(x);  x + mixer(BN(x));  x + fc2(GELU(fc1(BN(x))))."""

    def __init__(self, dim, mlp_ratio=4.):
        super().__init__()
        self.local_perception = _LocalIntegration(dim)
        self.norm1 = BatchNormWeights(dim)
        self.attn = AdditiveTokenMixer(dim)
        self.norm2 = BatchNormWeights(dim)
        self.mlp = _RCViTMlp(dim, int(dim * mlp_ratio))

    def tokens(self, x, B, H, W, training):
        li = self.local_perception.network
        x, h = Fh.fork(x, 2)
        h = _bn_act(Fh.linear(h, li[0].weight, li[0].bias), li[1], training, 0)
        h = Fh.dwconv3x3_gelu(h, li[2].weight, li[2].bias, B, H, W, True)
        x = Fh.linear(h, li[4].weight, li[4].bias, residual=x)
        x, h = Fh.fork(x, 2)
        x = Fh.add(x, self.attn.tokens(_bn_act(h, self.norm1, training, 0), B, H, W, training))
        x, h = Fh.fork(x, 2)
        f = Fh.gelu(Fh.linear(_bn_act(h, self.norm2, training, 0), self.mlp.fc1.weight, self.mlp.fc1.bias))
        return Fh.linear(f, self.mlp.fc2.weight, self.mlp.fc2.bias, residual=x)


class _RCViTEmbedding(nn.Module):
    """casvit.py:28-48 between stages: conv k3 s2 p1 (bias) + BatchNorm."""

    def __init__(self, c1, c2):
        super().__init__()
        self.proj = ConvWeights(c1, c2, 3, 2, 1)
        self.norm = BatchNormWeights(c2)


class RCViT(nn.Module):
    """models/backbones/casvit.py:181-278 with fork_feat=True as its factories build it: a two-convolution stem (k3 s2 p1 + BN + ReLU,
    twice), four stages of AdditiveBlocks with a k3 s2 p1 Embedding between them, and a BatchNorm norm{0,2,4,6} on the copy of each stage
    output that goes to the decode head (the un-normed tensor continues).  No drop path (the factories pass no rate), no dropout.
    Every conv and BatchNorm keeps torch's default initialisation (cls_init_weights touches nn.Linear only, :242-246)."""

    def __init__(self, layers, embed_dims, mlp_ratios=4):
        super().__init__()
        self.channels = list(embed_dims)
        self.compute_dtype = torch.bfloat16
        c0 = embed_dims[0]
        self.patch_embed = nn.Sequential(ConvWeights(3, c0 // 2, 3, 2, 1), BatchNormWeights(c0 // 2), nn.Identity(),
                                         ConvWeights(c0 // 2, c0, 3, 2, 1), BatchNormWeights(c0), nn.Identity())
        network = []
        for i in range(len(layers)):
            network.append(nn.Sequential(*[AdditiveBlock(embed_dims[i], mlp_ratios) for _ in range(layers[i])]))
            if i < len(layers) - 1:
                network.append(_RCViTEmbedding(embed_dims[i], embed_dims[i + 1]))
        self.network = nn.ModuleList(network)
        self.out_indices = [0, 2, 4, 6]
        for i_emb, i_layer in enumerate(self.out_indices):
            self.add_module(f'norm{i_layer}', BatchNormWeights(embed_dims[i_emb]))

    def forward_tokens(self, x):
        """x: fp32 NCHW image.  Returns 4 TokenMaps (strides 4/8/16/32)."""
        B, _, H, W = x.shape
        tr = self.training
        pe = self.patch_embed
        t = Fh.conv_patch(x, pe[0].weight, pe[0].bias, (B, H, W, 3, 3, 2, 1), image=True, dtype=self.compute_dtype)
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        t = _bn_act(t, pe[1], tr, 1)
        t = Fh.conv_patch(t, pe[3].weight, pe[3].bias, (B, H, W, pe[3].in_channels, 3, 2, 1))
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        t = _bn_act(t, pe[4], tr, 1)
        outs = []
        for idx, m in enumerate(self.network):
            if isinstance(m, _RCViTEmbedding):
                t = Fh.conv_patch(t, m.proj.weight, m.proj.bias, (B, H, W, m.proj.in_channels, 3, 2, 1))
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                t = _bn_act(t, m.norm, tr, 0)
                continue
            for blk in m:
                t = blk.tokens(t, B, H, W, tr)
            if idx != len(self.network) - 1:
                t, th = Fh.fork(t, 2)                # the stage output feeds its output norm and the next Embedding
            else:
                th = t
            outs.append(TokenMap(_bn_act(th, getattr(self, f'norm{idx}'), tr, 0), B, H, W))
        return outs

    def forward(self, x):
        return [tm.nchw() for tm in self.forward_tokens(x)]


# the reference's factories (casvit.py:283-313)
def rcvit_s(**kw):
    return RCViT(layers=[3, 3, 6, 3], embed_dims=[48, 64, 128, 256], **kw)


def rcvit_m(**kw):
    return RCViT(layers=[3, 3, 6, 3], embed_dims=[64, 96, 192, 384], **kw)


def rcvit_t(**kw):
    return RCViT(layers=[3, 3, 6, 3], embed_dims=[96, 128, 256, 512], **kw)


# ---- MetaFormer / ConvFormer (models/backbones/metaformer.py) ------------------------------------------------------------------
class _GainOnlyNorm(nn.Module):
    """LayerNormGeneral(bias=False) / LayerNormWithoutBias (metaformer.py:299-370): a LayerNorm over the channels with a gain and no
    bias, eps 1e-6.  State: `weight` alone.  It runs on the ordinary LayerNorm kernels fed a cached zero beta that is no parameter."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    forward = _no_forward


_ZERO_BETA = {}


def _zero_beta(C, device):
    """fp32 zeros [C] on `device`, made once per (C, device) -- outside any captured region, because the first pass of a train step
    is its warm-up -- and shared by every gain-only norm of that width.  Its gradient is discarded."""
    key = (int(C), str(device))
    z = _ZERO_BETA.get(key)
    if z is None:
        z = _ZERO_BETA[key] = torch.zeros(C, dtype=torch.float32, device=device)
    return z


class _StarReLUWeights(nn.Module):
    """StarReLU's parameters (metaformer.py:224-241): scale [1] = 1, bias [1] = 0."""

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))

    forward = _no_forward


class _ScaleWeights(nn.Module):
    """Scale (metaformer.py:198-208): scale [dim]."""

    def __init__(self, dim, init_value=1.0):
        super().__init__()
        self.scale = nn.Parameter(init_value * torch.ones(dim))

    forward = _no_forward


class _SepConv(nn.Module):
    """metaformer.py:373-400: Linear (x2, no bias) -> StarReLU -> depthwise 7 x 7 (no bias) -> Linear (no bias)."""

    def __init__(self, dim, expansion_ratio=2):
        super().__init__()
        med = int(expansion_ratio * dim)
        self.pwconv1 = LinearWeights(dim, med, bias=False)
        self.act1 = _StarReLUWeights()
        self.dwconv = ConvWeights(med, med, 7, 1, 3, groups=med, bias=False)
        self.pwconv2 = LinearWeights(med, dim, bias=False)


class _MetaFormerMlp(nn.Module):
    """metaformer.py:421-445 with drop = 0: Linear (x4, no bias) -> StarReLU -> Linear (no bias)."""

    def __init__(self, dim, mlp_ratio=4):
        super().__init__()
        self.fc1 = LinearWeights(dim, int(mlp_ratio * dim), bias=False)
        self.act = _StarReLUWeights()
        self.fc2 = LinearWeights(int(mlp_ratio * dim), dim, bias=False)


class _MlpHead(nn.Module):
    """metaformer.py:448-468, the classification head the factories build and forward() never runs: parameters only, so that the
    reference's checkpoints load strict."""

    def __init__(self, dim, num_classes=1000, mlp_ratio=4):
        super().__init__()
        self.fc1 = LinearWeights(dim, int(mlp_ratio * dim))
        self.norm = LayerNormWeights(int(mlp_ratio * dim))
        self.fc2 = LinearWeights(int(mlp_ratio * dim), num_classes)


class ConvFormerBlock(nn.Module):
    """MetaFormerBlock (metaformer.py:471-513) with token_mixer = SepConv, gain-only norms, no drop path and no layer scale:
    x = res_scale1(x) + SepConv(norm1(x));  x = res_scale2(x) + Mlp(norm2(x)).  res_scale{1,2} exist in stages 3 and 4 only.  The
    residual add stays in the epilogue of the branch's last product; a scaled skip path is the product's `residual=` operand, and its
    data gradient meets the branch's in the LayerNorm backward."""

    def __init__(self, dim, res_scale_init_value=None):
        super().__init__()
        self.dim = dim
        self.norm1 = _GainOnlyNorm(dim)
        self.token_mixer = _SepConv(dim)
        if res_scale_init_value:
            self.res_scale1 = _ScaleWeights(dim, res_scale_init_value)
        self.norm2 = _GainOnlyNorm(dim)
        self.mlp = _MetaFormerMlp(dim)
        if res_scale_init_value:
            self.res_scale2 = _ScaleWeights(dim, res_scale_init_value)

    def tokens(self, x, B, H, W):
        zb = _zero_beta(self.dim, x.device)
        tm, mlp = self.token_mixer, self.mlp
        x, h = Fh.layer_norm_res(x, self.norm1.weight, zb, self.norm1.eps)
        h = Fh.linear(h, tm.pwconv1.weight, None)
        h = Fh.star_relu(h, tm.act1.scale, tm.act1.bias)
        h = Fh.dwconv7x7(h, tm.dwconv.weight, None, B, H, W)
        res = Fh.col_scale(x, self.res_scale1.scale) if hasattr(self, 'res_scale1') else x
        x = Fh.linear(h, tm.pwconv2.weight, None, residual=res)
        x, h = Fh.layer_norm_res(x, self.norm2.weight, zb, self.norm2.eps)
        h = Fh.linear(h, mlp.fc1.weight, None)
        h = Fh.star_relu(h, mlp.act.scale, mlp.act.bias)
        res = Fh.col_scale(x, self.res_scale2.scale) if hasattr(self, 'res_scale2') else x
        return Fh.linear(h, mlp.fc2.weight, None, residual=res)


class _MetaFormerDownsampling(nn.Module):
    """metaformer.py:172-195: [gain-only norm ->] conv (bias) [-> gain-only norm]; registration order pre_norm, conv, post_norm."""

    def __init__(self, c1, c2, k, s, p, pre_norm=False, post_norm=False):
        super().__init__()
        if pre_norm:
            self.pre_norm = _GainOnlyNorm(c1)
        self.conv = ConvWeights(c1, c2, k, s, p)
        if post_norm:
            self.post_norm = _GainOnlyNorm(c2)


class MetaFormer(nn.Module):
    """models/backbones/metaformer.py:532-683 as the convformer_* factories build it: stem conv k7 s4 p2 (bias) + gain-only LayerNorm,
    three [gain-only LayerNorm + conv k3 s2 p1 (bias)] downsamplers, four stages of ConvFormerBlocks with the residual scale (init 1.0)
    in stages 3 and 4, and the four stage outputs without an output norm (forward_intermediates).  `norm` and `head` (MlpHead) are the
    reference's unused classification tail: parameters that never receive a gradient.  No drop path (the factories pass no rate)."""

    def __init__(self, depths, dims, res_scale_init_values=(None, None, 1.0, 1.0), num_classes=1000):
        super().__init__()
        from .containers import trunc_normal_
        self.channels = list(dims)
        self.depths = list(depths)
        self.compute_dtype = torch.bfloat16
        down = [3] + list(dims)
        self.downsample_layers = nn.ModuleList(
            [_MetaFormerDownsampling(down[0], down[1], 7, 4, 2, post_norm=True)] +
            [_MetaFormerDownsampling(down[i], down[i + 1], 3, 2, 1, pre_norm=True) for i in range(1, 4)])
        self.stages = nn.ModuleList(
            [nn.Sequential(*[ConvFormerBlock(dims[i], res_scale_init_values[i]) for _ in range(depths[i])]) for i in range(4)])
        self.norm = LayerNormWeights(dims[-1], eps=1e-6)
        self.head = _MlpHead(dims[-1], num_classes)
        for m in self.modules():                                # _init_weights (:632-636)
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward_tokens(self, x):
        """x: fp32 NCHW image.  Returns 4 TokenMaps (strides 4/8/16/32)."""
        B, _, H, W = x.shape
        outs = []
        t = None
        for i in range(4):
            ds = self.downsample_layers[i]
            if i == 0:
                t = Fh.conv_patch(x, ds.conv.weight, ds.conv.bias, (B, H, W, 3, 7, 4, 2), image=True, dtype=self.compute_dtype)
                H, W = (H + 4 - 7) // 4 + 1, (W + 4 - 7) // 4 + 1
                t = Fh.layer_norm(t, ds.post_norm.weight, _zero_beta(self.channels[0], t.device), ds.post_norm.eps)
            else:
                t = Fh.layer_norm(t, ds.pre_norm.weight, _zero_beta(self.channels[i - 1], t.device), ds.pre_norm.eps)
                t = Fh.conv_patch(t, ds.conv.weight, ds.conv.bias, (B, H, W, self.channels[i - 1], 3, 2, 1))
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            for blk in self.stages[i]:
                t = blk.tokens(t, B, H, W)
            if i < 3:
                t, th = Fh.fork(t, 2)                # the stage output goes to the decode head and into the next downsampler's norm
            else:
                th = t
            outs.append(TokenMap(th, B, H, W))
        return outs

    def forward(self, x):
        return [tm.nchw() for tm in self.forward_tokens(x)]


# the reference's ConvFormer factories (metaformer.py:926-1243); the suffixed names differ in their pretrained checkpoint alone
CONVFORMER_SETTINGS = {
    'convformer_s18': ([3, 3, 9, 3], [64, 128, 320, 512]),
    'convformer_s36': ([3, 12, 18, 3], [64, 128, 320, 512]),
    'convformer_m36': ([3, 12, 18, 3], [96, 192, 384, 576]),
    'convformer_b36': ([3, 12, 18, 3], [128, 256, 512, 768]),
}
CONVFORMER_SUFFIXES = ('', '_384', '_in21ft1k', '_384_in21ft1k', '_in21k')


def _convformer_factory(base):
    depths, dims = CONVFORMER_SETTINGS[base]

    def factory(**kw):
        return MetaFormer(depths=depths, dims=dims, **kw)
    return factory


for _base in CONVFORMER_SETTINGS:
    for _sfx in CONVFORMER_SUFFIXES:
        globals()[_base + _sfx] = _convformer_factory(_base)
        globals()[_base + _sfx].__name__ = _base + _sfx
del _base, _sfx
