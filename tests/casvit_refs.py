"""Float64 restatements of the CAS-ViT token-mixer kernels (csrc/token_mixer.hip; formulas of include/segfac.h) and of the whole
AdditiveTokenMixer built from them (models/backbones/casvit.py:68-92, 112-138) with BatchNorm in training mode.

The kernel formulas are written out forward AND backward; `mixer` chains them through torch.autograd.Function wrappers, so its input
gradient runs through the restated backward formulas and not through autograd's own derivative of the forward ones.  The 1 x 1 and
depthwise convolutions and the BatchNorms in between are torch's, in float64."""
import torch
import torch.nn.functional as F


# ---- the three kernel pairs on [M = B HW, C] float64 tensors ---------------------------------------------------------------------------
def spatial_gate_fwd(x, r, w, B):
    """-> (y, s, pool): s[m] = sigmoid(sum_c r[m, c] w[c]), y = x * s, pool[b, c] = sum over the pixels of sample b of x * s."""
    M, C = x.shape
    s = torch.sigmoid(r @ w)
    y = x * s[:, None]
    return y, s, y.view(B, M // B, C).sum(1)


def spatial_gate_bwd(dy, dpool, x, r, s, w, B):
    """-> (dx, dr, dw)"""
    M, C = x.shape
    g = dy if dpool is None else dy + dpool.repeat_interleave(M // B, 0)
    dx = g * s[:, None]
    ds = (g * x).sum(1)
    dl = ds * s * (1 - s)
    return dx, dl[:, None] * w[None, :], (dl[:, None] * r).sum(0)


def channel_gate_mix_fwd(q1, k1, gq, gk):
    B, HW = gq.shape[0], q1.shape[0] // gq.shape[0]
    return q1 * gq.repeat_interleave(HW, 0) + k1 * gk.repeat_interleave(HW, 0)


def channel_gate_mix_bwd(du, q1, k1, gq, gk):
    """-> (dq1, dk1, dgq, dgk)"""
    B, C = gq.shape
    HW = q1.shape[0] // B
    return (du * gq.repeat_interleave(HW, 0), du * gk.repeat_interleave(HW, 0), (du * q1).view(B, HW, C).sum(1),
            (du * k1).view(B, HW, C).sum(1))


def gated_mul_fwd(a, v):
    return a * v


def gated_mul_bwd(dz, a, v):
    """-> (da, dv)"""
    return dz * v, dz * a


# ---- the composed mixer ------------------------------------------------------------------------------------------------------------------
class _SpatialGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, w, B):
        y, s, pool = spatial_gate_fwd(x, r, w, B)
        ctx.save_for_backward(x, r, s, w)
        ctx.B = B
        return y, pool

    @staticmethod
    def backward(ctx, dy, dpool):
        x, r, s, w = ctx.saved_tensors
        return spatial_gate_bwd(dy, dpool, x, r, s, w, ctx.B) + (None,)


class _ChannelGateMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q1, k1, gq, gk):
        ctx.save_for_backward(q1, k1, gq, gk)
        return channel_gate_mix_fwd(q1, k1, gq, gk)

    @staticmethod
    def backward(ctx, du):
        return channel_gate_mix_bwd(du, *ctx.saved_tensors)


class _GatedMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, v):
        ctx.save_for_backward(a, v)
        return gated_mul_fwd(a, v)

    @staticmethod
    def backward(ctx, dz):
        return gated_mul_bwd(dz, *ctx.saved_tensors)


def _dw3x3(t, weight, bias, B, H, W):
    """depthwise 3 x 3, pad 1, on tokens [B H W, C]"""
    C = t.shape[1]
    y = F.conv2d(t.view(B, H, W, C).permute(0, 3, 1, 2), weight, bias, 1, 1, 1, C)
    return y.permute(0, 2, 3, 1).reshape(B * H * W, C)


def _bn_train(t, weight, bias, eps=1e-5):
    """BatchNorm2d with batch statistics on tokens: per-channel statistics over all rows"""
    mean, var = t.mean(0), t.var(0, unbiased=False)
    return (t - mean) * torch.rsqrt(var + eps) * weight + bias


def mixer(x, sd, dy=None):
    """AdditiveTokenMixer.forward in train mode on an NCHW input, float64; sd: the module's state_dict (tools/make_casvit_goldens.py:
    mixer_inventory).  -> y (NCHW), and the input gradient for the output gradient dy when one is given."""
    sd = {k: v.double() for k, v in sd.items()}
    B, C, H, W = x.shape
    xin = x.double().requires_grad_(dy is not None)
    t = xin.permute(0, 2, 3, 1).reshape(B * H * W, C)
    q, k, v = (t @ sd['qkv.weight'].view(3 * C, C).t()).chunk(3, dim=1)

    def oper(name, z):
        r = _dw3x3(z, sd[f'{name}.0.block.0.weight'], sd[f'{name}.0.block.0.bias'], B, H, W)
        r = torch.relu(_bn_train(r, sd[f'{name}.0.block.1.weight'], sd[f'{name}.0.block.1.bias']))
        y, pool = _SpatialGate.apply(z, r, sd[f'{name}.0.block.3.weight'].view(C), B)
        return y, torch.sigmoid((pool / (H * W)) @ sd[f'{name}.1.block.1.weight'].view(C, C).t())
    q1, gq = oper('oper_q', q)
    k1, gk = oper('oper_k', k)
    u = _ChannelGateMix.apply(q1, k1, gq, gk)
    a = _dw3x3(u, sd['dwc.weight'], sd['dwc.bias'], B, H, W)
    z = _GatedMul.apply(a, v)
    y = _dw3x3(z, sd['proj.weight'], sd['proj.bias'], B, H, W).view(B, H, W, C).permute(0, 3, 1, 2)
    if dy is None:
        return y.detach(), None
    y.backward(dy.double())
    return y.detach(), xin.grad.detach()
