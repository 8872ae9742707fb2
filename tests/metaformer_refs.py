"""Float64 restatements of the MetaFormer kernels (csrc/metaformer.hip; formulas of include/segfac.h) and of the whole ConvFormer block
built from them (models/backbones/metaformer.py:471-513 with token_mixer = SepConv and gain-only LayerNorms).

The functions take and return torch tensors of any floating dtype (float64 in the tests); nothing here touches a GPU.  The block is pinned
to the reference by tests/test_convformer_cpu.py against tests/golden/convformer_block_cases.npz; the GPU kernels are then held to these
functions."""
import torch
import torch.nn.functional as F


def starrelu_fwd(u, s, b):
    """y = s * max(u, 0)^2 + b; s, b: one-element tensors"""
    return s * torch.relu(u) ** 2 + b


def starrelu_bwd(dy, u, s):
    """-> (du = dy * 2 s max(u, 0), ds = sum dy max(u, 0)^2, db = sum dy)"""
    p = torch.relu(u)
    return dy * (2 * s * p), (dy * p * p).sum().reshape(1), dy.sum().reshape(1)


def starrelu_sum_terms(dy, u):
    """(sum |dy max(u, 0)^2|, sum |dy|): the scales of the two sums' error bars"""
    p = torch.relu(u)
    return (dy * p * p).abs().sum().item(), dy.abs().sum().item()


def colscale_fwd(x, scale):
    return x * scale


def colscale_bwd(dy, x, scale):
    """-> (dx = dy * scale[c], dscale[c] = sum_rows dy * x)"""
    return dy * scale, (dy * x).sum(0)


class StarReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, s, b):
        ctx.save_for_backward(u, s)
        return starrelu_fwd(u, s, b)

    @staticmethod
    def backward(ctx, dy):
        u, s = ctx.saved_tensors
        return starrelu_bwd(dy, u, s)


class ColScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.save_for_backward(x, scale)
        return colscale_fwd(x, scale)

    @staticmethod
    def backward(ctx, dy):
        x, scale = ctx.saved_tensors
        return colscale_bwd(dy, x, scale)


def block(x, sd, dy, eps=1e-6):
    """One ConvFormer block on x [B, H, W, C] with the state dict sd of the reference's MetaFormerBlock (res_scale{1,2}.scale present or
    not), in float64: -> (y, dx, {parameter name: gradient}) for the output gradient dy.  StarReLU and the residual scale run through the
    hand-written forward / backward pairs above; LayerNorm, the Linears and the depthwise convolution are torch's."""
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    x = x.double().clone().requires_grad_(True)
    B, H, W, C = x.shape

    def skip(t, key):
        if key in p:
            return ColScale.apply(t.reshape(-1, C), p[key]).reshape(t.shape)
        return t
    h = F.layer_norm(x, (C,), p['norm1.weight'], None, eps)
    h = h @ p['token_mixer.pwconv1.weight'].t()
    h = StarReLU.apply(h, p['token_mixer.act1.scale'], p['token_mixer.act1.bias'])
    h = F.conv2d(h.permute(0, 3, 1, 2), p['token_mixer.dwconv.weight'], None, padding=3, groups=2 * C).permute(0, 2, 3, 1)
    x1 = skip(x, 'res_scale1.scale') + h @ p['token_mixer.pwconv2.weight'].t()
    h = F.layer_norm(x1, (C,), p['norm2.weight'], None, eps)
    h = StarReLU.apply(h @ p['mlp.fc1.weight'].t(), p['mlp.act.scale'], p['mlp.act.bias'])
    y = skip(x1, 'res_scale2.scale') + h @ p['mlp.fc2.weight'].t()
    y.backward(dy.double())
    return y.detach(), x.grad, {k: v.grad for k, v in p.items()}
