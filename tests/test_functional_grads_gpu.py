"""The autograd Functions of segmentation_factory_amd.functional one at a time, under the three ways a parameter gradient leaves a backward:

  (a) plain autograd: no flat-gradient slots, gradients arrive in `.grad`
  (b) direct placement: a FusedAGCAdamW over the case's parameters, enable_direct_grads() + begin_backward(); gradients read from the slots
  (c) as (b) with the backward inside `functional.defer_weight_grads()` (grouped dW / db products, grouped finalizes)

Per case: outputs and input gradients torch.equal across the regimes; in (b) and (c) no `.grad`, every slot delivered exactly once (a
second delivery raises in the optimizer's bookkeeping, a missing one leaves the set of delivered slots short) and nothing left in
`_SCALED_DY`; parameter gradients of (b) and (c) torch.equal to those of (a).

Recorded on the MI355X with the glue as it stood before it was gathered into shared helpers: every parameter gradient of every case
below was bit-equal between (a), (b) and (c), so no case needs the looser float64 rule of
tests/test_ln_linear_bwd_gpu.py::_check_params and all of them assert torch.equal."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

def _param(g, *shape, scale=0.2, shift=0.0):
    return torch.nn.Parameter((torch.randn(*shape, generator=g) * scale + shift).cuda())


def _act(g, *shape, dtype=torch.bfloat16, grad=True):
    return torch.randn(*shape, generator=g).cuda().to(dtype).requires_grad_(grad)


def _rscale(n=2):
    return torch.tensor([1.0 / 0.9, 1.0 / 0.8, 1.0 / 0.7][:n], device='cuda')


def _norm_params(g, C, prefix=''):
    return {prefix + 'gamma': _param(g, C, scale=0.3, shift=1.0), prefix + 'beta': _param(g, C)}


# ---- the cases: build(g, Fh) -> (parameters by name, in flat-buffer order; activations that take a gradient; forward() -> outputs) -----
def _linear(dtype, bias, res):
    def build(g, Fh):
        p = {'w': _param(g, 32, 32)}
        if bias:
            p['b'] = _param(g, 32)
        acts = [_act(g, 64, 32, dtype=dtype)]
        r = rs = None
        if res:
            r, rs = _act(g, 64, 32, dtype=dtype), _rscale()
            acts.append(r)
        return p, acts, lambda: (Fh.linear(acts[0], p['w'], p.get('b'), residual=r, rscale=rs, rows_per_group=32 if res else None),)
    return build


def _linear_fork(g, Fh):
    p = {'w': _param(g, 32, 32), 'b': _param(g, 32)}
    x = _act(g, 64, 32)
    return p, [x], lambda: Fh.linear_fork(x, p['w'], p['b'])


def _qkv_split3(g, Fh):
    p = {'w': _param(g, 96, 32)}
    x = _act(g, 64, 32)
    return p, [x], lambda: Fh.qkv_split3(x, p['w'])


def _conv_patch(k, s, pad, image):
    def build(g, Fh):
        cin, hw = (3, 16) if image else (8, 8)
        p = {'w': _param(g, 16, cin, k, k), 'b': _param(g, 16)}
        x = _act(g, 1, 3, 16, 16, dtype=torch.float32, grad=False) if image else _act(g, hw * hw, cin)
        return p, ([] if image else [x]), lambda: (Fh.conv_patch(x, p['w'], p['b'], (1, hw, hw, cin, k, s, pad), image=image,
                                                                 dtype=torch.bfloat16),)
    return build


def _ln_patch_conv_from_col(g, Fh):
    C, W, sr = 32, 8, 2
    assert Fh.patch_layout_ok(W, W, sr)
    p = dict(_norm_params(g, C), w=_param(g, C, C, sr, sr), b=_param(g, C))
    x = _act(g, W * W, C)

    def fwd():
        x2, h, col = Fh.layer_norm_res_patch(x, p['gamma'], p['beta'], 1e-5, W, sr)
        return x2, h, Fh.conv_from_col(col, p['w'], p['b'], sr)
    return p, [x], fwd


def _conv3x3(dtype, dilation):
    def build(g, Fh):
        p = {'w': _param(g, 8, 8, 3, 3)}
        x = _act(g, 64, 8, dtype=dtype)
        if dilation > 1:
            return p, [x], lambda: (Fh.conv3x3_dilated(x, p['w'], 1, 8, 8, dilation),)
        return p, [x], lambda: (Fh.conv3x3(x, p['w'], 1, 8, 8),)
    return build


def _layer_norm(kind, after_linear):
    """kind: layer_norm / layer_norm_res / layer_norm_fork at 64 x 32; after_linear: the input is the output of linear(..., residual, rscale),
    whose backward collects the DropPath-scaled gradient the LayerNorm backward parks"""
    def build(g, Fh):
        p = _norm_params(g, 32)
        x = _act(g, 64, 32)
        acts = [x]
        if after_linear:
            p.update(w=_param(g, 32, 32), b=_param(g, 32))
            r, rs = _act(g, 64, 32), _rscale()
            acts.append(r)

        def fwd():
            t = Fh.linear(x, p['w'], p['b'], residual=r, rscale=rs, rows_per_group=32) if after_linear else x
            out = getattr(Fh, kind)(t, p['gamma'], p['beta'], 1e-5)
            return out if isinstance(out, tuple) else (out,)
        return p, acts, fwd
    return build


def _dwconv3x3_gelu(g, Fh):
    p = {'w': _param(g, 32, 1, 3, 3), 'b': _param(g, 32)}
    x = _act(g, 64, 32)
    return p, [x], lambda: (Fh.dwconv3x3_gelu(x, p['w'], p['b'], 1, 8, 8, True),)


def _ln_res_linear(g, Fh):
    """(37, 32) -> 128, the smallest shape of tests/test_ln_linear_bwd_gpu.py, behind a residual Linear with DropPath scales"""
    rows, C = 37, 32
    p = dict(w0=_param(g, C, C), b0=_param(g, C), **_norm_params(g, C), w=_param(g, 4 * C, C), b=_param(g, 4 * C))
    x, r, rs = _act(g, rows, C), _act(g, rows, C), _rscale(3)

    def fwd():
        t = Fh.linear(x, p['w0'], p['b0'], residual=r, rscale=rs, rows_per_group=13)
        assert Fh.layer_norm_res_linear_ok(t, p['gamma'], p['beta'], p['w'], p['b'])
        return Fh.layer_norm_res_linear(t, p['gamma'], p['beta'], 1e-5, p['w'], p['b'])
    return p, [x, r], fwd


def _ln_res_patch_linear(g, Fh):
    """C = 32 on the (2, 16, 32) map with sr = 8 of tests/test_ln_linear_fwd_gpu.py (PATCH[32]), behind a residual Linear with DropPath scales"""
    B, H, W, sr, C = 2, 16, 32, 8, 32
    rows = B * H * W
    p = dict(w0=_param(g, C, C), b0=_param(g, C), **_norm_params(g, C), w=_param(g, C, C), b=_param(g, C))
    x, r, rs = _act(g, rows, C), _act(g, rows, C), _rscale()

    def fwd():
        t = Fh.linear(x, p['w0'], p['b0'], residual=r, rscale=rs, rows_per_group=H * W)
        assert Fh.patch_layout_ok(W, H, sr) and Fh.layer_norm_res_patch_linear_ok(t, p['gamma'], p['beta'], p['w'], p['b'])
        return Fh.layer_norm_res_patch_linear(t, p['gamma'], p['beta'], 1e-5, W, sr, p['w'], p['b'])
    return p, [x, r], fwd


def _dwconv3x3_gelu_linear(g, Fh):
    """(2, 5, 16, 128, 32), the smallest case of tests/test_ffn_bwd_fused_gpu.py, with residual + DropPath scales and a LayerNorm behind it
    (whose backward parks the scaled gradient this Function's backward collects)"""
    B, H, W, Cc, Cin = 2, 5, 16, 128, 32
    p = dict(w2=_param(g, Cin, Cc), b2=_param(g, Cin), w=_param(g, Cc, 1, 3, 3, scale=0.3), b=_param(g, Cc), **_norm_params(g, Cin))
    x, r, rs = _act(g, B * H * W, Cc), _act(g, B * H * W, Cin), _rscale()

    def fwd():
        assert Fh.dwconv3x3_gelu_linear_ok(x, p['w2'], p['b2'], p['w'], p['b'], B, H, W)
        y = Fh.dwconv3x3_gelu_linear(x, p['w2'], p['b2'], p['w'], p['b'], B, H, W, residual=r, rscale=rs)
        return (Fh.layer_norm(y, p['gamma'], p['beta'], 1e-5),)
    return p, [x, r], fwd


BF16, F32 = torch.bfloat16, torch.float32
LN_FUSED = {'SEGFAC_LN_LINEAR_FWD_FUSED': '2', 'SEGFAC_LN_LINEAR_BWD_FUSED': '2'}
CASES = {
    'linear-bf16': (_linear(BF16, True, False), {}),
    'linear-fp32': (_linear(F32, True, False), {}),
    'linear-nobias-bf16': (_linear(BF16, False, False), {}),
    'linear-nobias-fp32': (_linear(F32, False, False), {}),
    'linear-residual-bf16': (_linear(BF16, True, True), {}),
    'linear-residual-fp32': (_linear(F32, True, True), {}),
    'linear_fork': (_linear_fork, {}),
    'qkv_split3': (_qkv_split3, {}),
    'conv_patch-k2s2': (_conv_patch(2, 2, 0, False), {}),
    'conv_patch-k3s2p1': (_conv_patch(3, 2, 1, False), {}),
    'conv_patch-image-k7s4p3': (_conv_patch(7, 4, 3, True), {}),
    'layer_norm_res_patch-conv_from_col': (_ln_patch_conv_from_col, {}),
    'conv3x3-bf16': (_conv3x3(BF16, 1), {}),
    'conv3x3-fp32': (_conv3x3(F32, 1), {}),                       # (fp32: ConvPatchFn without bias)
    'conv3x3_dilated': (_conv3x3(BF16, 2), {}),
    'layer_norm': (_layer_norm('layer_norm', False), {}),
    'layer_norm_res': (_layer_norm('layer_norm_res', False), {}),
    'layer_norm_fork': (_layer_norm('layer_norm_fork', False), {}),
    'linear-layer_norm': (_layer_norm('layer_norm', True), {}),
    'linear-layer_norm_res': (_layer_norm('layer_norm_res', True), {}),
    'linear-layer_norm_fork': (_layer_norm('layer_norm_fork', True), {}),
    'dwconv3x3_gelu': (_dwconv3x3_gelu, {}),
    'layer_norm_res_linear': (_ln_res_linear, LN_FUSED),
    'layer_norm_res_patch_linear-one_pass': (_ln_res_patch_linear, LN_FUSED),
    'layer_norm_res_patch_linear-three_launches': (_ln_res_patch_linear, {'SEGFAC_LN_LINEAR_FWD_FUSED': '2', 'SEGFAC_LN_LINEAR_BWD_FUSED': '0'}),
    'dwconv3x3_gelu_linear': (_dwconv3x3_gelu_linear, {'SEGFAC_FFN_BWD_FUSED': '2', 'SEGFAC_DW_NO_SMALL': '1'}),
}


def _run(build, regime):
    """-> (outputs, input gradients, parameter gradients by name) of one forward + backward on the case's seeded tensors"""
    from segmentation_factory_amd import functional as Fh
    from segmentation_factory_amd.optim import FusedAGCAdamW
    params, acts, fwd = build(torch.Generator().manual_seed(1234), Fh)
    opt = None
    if regime != 'a':
        opt = FusedAGCAdamW([{'params': list(params.values()), 'weight_decay': 0.0}], lr=1e-3)
        opt.enable_direct_grads()
        opt.begin_backward()
    outs = fwd()
    gd = torch.Generator().manual_seed(99)
    douts = [torch.randn(o.shape, generator=gd).cuda().to(o.dtype) for o in outs]
    with (Fh.defer_weight_grads() if regime == 'c' else contextlib.nullcontext()):
        torch.autograd.backward(outs, douts)
    torch.cuda.synchronize()
    assert Fh._SCALED_DY == {}
    assert all(a.grad is not None for a in acts)
    if opt is None:
        grads = {k: p.grad.clone() for k, p in params.items()}
    else:
        assert all(p.grad is None for p in params.values())
        assert set(opt._written) == {p._segf_grad.data_ptr() for p in params.values()} and len(opt._written) == len(params)
        grads = {k: p._segf_grad.clone() for k, p in params.items()}
        opt.disable_direct_grads()
    return [o.detach().clone() for o in outs], [a.grad.clone() for a in acts], grads


@pytest.mark.parametrize('name', list(CASES))
def test_the_three_ways_a_parameter_gradient_leaves_a_backward(name, monkeypatch):
    build, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (ya, dxa, ga), rb, rc = (_run(build, r) for r in 'abc')
    bad = []
    for regime, (y, dx, grads) in (('b', rb), ('c', rc)):
        assert len(y) == len(ya) and all(torch.equal(u, v) for u, v in zip(y, ya)), (name, regime, 'outputs')
        assert len(dx) == len(dxa) and all(torch.equal(u, v) for u, v in zip(dx, dxa)), (name, regime, 'input gradients')
        assert set(grads) == set(ga)
        for k, gr in grads.items():
            same = torch.equal(gr, ga[k])
            print(f'{name} ({regime}) {k}: {"bit-equal to (a)" if same else f"unequal elements {(gr != ga[k]).sum().item()} of {gr.numel()}"}')
            assert torch.isfinite(gr).all() and gr.abs().sum().item() > 0
            if not same:
                bad.append((regime, k, (gr - ga[k]).abs().max().item()))
    assert not bad, (name, bad)


# ---- where BatchNorm's (mean, rstd) come from -----------------------------------------------------------------------------------------
# Bounds, from the number formats alone (u = 2^-24, fp32; any summation order of n fp32 terms is within n u sum|t| of the exact sum):
#   mean    |err| <= n u max|x|                          (the sum of n values, divided by n)
#   var     |err| <= 2 n u max|x|^2 + 2 |mean| err(mean) (E[x^2] - mean^2 in fp32)   ->   rstd relative error <= err(var) / (2 var) + 4 u
#   pre_sums given: the two sums are the float64 sums rounded once, n in the bounds becomes 2
# bf16 output: |y - exact| <= 2^-8 |exact| + the fp32 slack of the affine map.
U = 2.0 ** -24
MOMENTUM, EPS = 0.1, 1e-5


def _bn_stat_bounds(x64, n_eff):
    amax, mean, var = x64.abs().max().item(), x64.mean(0), x64.var(0, unbiased=False)
    e_mean = n_eff * U * amax
    e_var = 2 * n_eff * U * amax * amax + 2 * mean.abs() * e_mean
    return mean, var, e_mean, e_var


def _bn_case(fn, mode, Fh, hip):
    fused = fn == 'bn_act_linear'
    M, K, N, rps = (32768, 64, 6, 16384) if fused else (64, 32, 6, 32)           # fused: the smallest rows segf_gemm_pro takes for both products
    Np = 8                                                                        # (the classifier's padded width, as the heads call it)
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(torch.bfloat16).cuda().requires_grad_()
    gam, bet = _param(g, K, scale=0.2, shift=1.0), _param(g, K, scale=0.1)
    w, b = _param(g, N, K, scale=K ** -0.5), _param(g, N)
    rm, rv = (0.1 * torch.randn(K, generator=g)).cuda(), (1.0 + 0.2 * torch.rand(K, generator=g)).cuda()
    rm0, rv0 = rm.clone(), rv.clone()
    x64 = x.detach().double()
    sums = torch.stack([x64.sum(0), (x64 * x64).sum(0)]).float() if mode == 'pre_sums' else None
    training = mode != 'eval'
    if fused:
        assert hip.gemm_pro_supported(torch.bfloat16, 0, M, Np, K, rps) and hip.gemm_pro_supported(torch.bfloat16, 2, Np, K, M, rps)
        y = Fh.bn_act_linear(x, gam, bet, rm, rv, training, MOMENTUM, EPS, 1, None, rps, w, b, pad_to=Np, pre_sums=sums)
        assert type(y.grad_fn).__name__.startswith('BnActLinearFn')
    else:
        y = Fh.batch_norm_act(x, gam, bet, rm, rv, training, MOMENTUM, EPS, 1, None, rps, pre_sums=sums)
    mean, rstd = y.grad_fn.saved_tensors[1:3]
    return dict(x64=x64, gam=gam, bet=bet, w=w, b=b, rm=rm, rv=rv, rm0=rm0, rv0=rv0, y=y, mean=mean, rstd=rstd, M=M, fused=fused)


@pytest.mark.parametrize('mode', ['pre_sums', 'batch', 'eval'])
@pytest.mark.parametrize('fn', ['batch_norm_act', 'bn_act_linear'])
def test_batch_norm_statistics_source(fn, mode):
    from segmentation_factory_amd import functional as Fh, hip
    t = _bn_case(fn, mode, Fh, hip)
    x64, mean, rstd, M = t['x64'], t['mean'], t['rstd'], t['M']
    torch.cuda.synchronize()
    if mode == 'eval':
        # the running buffers as they stand, untouched
        assert torch.equal(mean, t['rm0']) and torch.equal(rstd, torch.rsqrt(t['rv0'] + EPS))
        assert torch.equal(t['rm'], t['rm0']) and torch.equal(t['rv'], t['rv0'])
    else:
        m64, v64, e_mean, e_var = _bn_stat_bounds(x64, 2 if mode == 'pre_sums' else M)
        r64 = (v64 + EPS).rsqrt()
        d_mean, d_rstd = (mean.double() - m64).abs(), (rstd.double() - r64).abs() / r64
        print(f'{fn} {mode}: mean err {d_mean.max().item():.3e} (bound {e_mean:.3e}), rstd rel err {d_rstd.max().item():.3e} '
              f'(bound {(e_var / (2 * v64) + 4 * U).max().item():.3e})')
        assert (d_mean <= e_mean + 2 * U * m64.abs()).all()
        assert (d_rstd <= e_var / (2 * v64) + 4 * U).all()
        # running = (1 - momentum) * running + momentum * (batch mean, unbiased batch variance)   (torch.nn.BatchNorm2d)
        rm64 = (1 - MOMENTUM) * t['rm0'].double() + MOMENTUM * m64
        rv64 = (1 - MOMENTUM) * t['rv0'].double() + MOMENTUM * v64 * M / (M - 1)
        assert ((t['rm'].double() - rm64).abs() <= MOMENTUM * e_mean + 4 * U * rm64.abs()).all()
        assert ((t['rv'].double() - rv64).abs() <= MOMENTUM * e_var * M / (M - 1) + 4 * U * rv64.abs()).all()
    # the output from the statistics the Function saved
    a64 = ((x64 - mean.double()) * rstd.double() * t['gam'].detach().double() + t['bet'].detach().double()).clamp_min(0)
    y = t['y'].detach().double()
    if t['fused']:
        # operands rounded to bf16 (a rounding of the normalised value may fall either way: 2^-8 per term), fp32 sums, bf16 output
        w64 = t['w'].detach().to(torch.bfloat16).double()
        want = a64.to(torch.bfloat16).double() @ w64.t() + t['b'].detach().double()
        tol = 2.0 ** -7 * (a64 @ w64.abs().t()) + 2.0 ** -8 * want.abs() + 1e-5
    else:
        scale = rstd.double() * t['gam'].detach().double().abs()
        want, tol = a64, 2.0 ** -8 * a64 + 8 * U * ((x64.abs() + mean.double().abs()) * scale + t['bet'].detach().double().abs() + 1)
    print(f'{fn} {mode}: output max err {(y - want).abs().max().item():.3e}, largest err / bound {((y - want).abs() / tol).max().item():.3f}')
    assert ((y - want).abs() <= tol).all()
    if fn == 'bn_act_linear' and mode != 'eval':
        # the same kernels on the same operands as BatchNormActFn's: the two Functions agree on the statistics and the buffers to the bit
        x = x64.to(torch.bfloat16)
        rm, rv = t['rm0'].clone(), t['rv0'].clone()
        sums = torch.stack([x64.sum(0), (x64 * x64).sum(0)]).float() if mode == 'pre_sums' else None
        y2 = Fh.batch_norm_act(x.requires_grad_(), t['gam'], t['bet'], rm, rv, True, MOMENTUM, EPS, 1, None, 16384, pre_sums=sums)
        mean2, rstd2 = y2.grad_fn.saved_tensors[1:3]
        assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and torch.equal(rm, t['rm']) and torch.equal(rv, t['rv'])
