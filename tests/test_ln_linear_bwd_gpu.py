"""The backward of `norm2 -> mlp.fc1` in one pass (segf_layernorm_linear_bwd, ln_linear_bwd_kernel) against the three launches it replaces:
segf_gemm (layout 1) for fc1's data gradient, segf_layernorm_bwd_scaled, segf_gemm_dw_db.

  dy, dx, dxs                  torch.equal to the three-launch form
  dW1, db1, dgamma, dbeta      another summation order: both forms against a float64 oracle on the same bf16 inputs (the oracle LayerNorm
                               takes the bf16-rounded dy); per tensor the fused form's largest error is at most 2 x the three-launch
                               form's own (both sum the same products in fp32, in different trees)

Measured on the MI355X (largest error of the fused form / of the three-launch form, worst case over the kernel and Block cases
below): dW1 1.33, db1 1.58, dgamma 1.63, dbeta 1.00; dy, dx, dxs: no unequal element in any case."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1620, 32), (1620, 64), (37, 32), (64, 64)]          # 1620 = 3 samples x 540 rows: ragged last tile, 26 workgroups' partials
# ... and the row counts from which segf_gemm forms the data gradient with another kernel (the streaming kernels: 16384 rows at
# C = 32, 65536 at C = 64, where the K = 256 sum becomes four K-quarter partials), each with a ragged tail
THRESHOLDS = [(16384 + 37, 32), (65536 + 37, 64)]


@functools.lru_cache(maxsize=None)
def _inputs(rows, C):
    from segmentation_factory_amd import hip
    g = torch.Generator(device='cuda').manual_seed(1000 * C + rows)
    rn = lambda *s: torch.randn(*s, generator=g, device='cuda')      # noqa: E731
    x = (rn(rows, C) * 1.5 + 0.3).to(torch.bfloat16)
    gamma, beta = 1.0 + 0.3 * rn(C), 0.2 * rn(C)
    w1 = (rn(4 * C, C) * 0.2).to(torch.bfloat16)
    dh = rn(rows, 4 * C).to(torch.bfloat16)
    dres = rn(rows, C).to(torch.bfloat16)
    y, mean, rstd = hip.layernorm_fwd(x, gamma, beta, 1e-5)
    groups = 3
    rpg = (rows + groups - 1) // groups
    rscale = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9], device='cuda')          # the second sample is dropped
    return dict(x=x, gamma=gamma, w1=w1, dh=dh, dres=dres, y=y, mean=mean, rstd=rstd, rscale=rscale, rpg=rpg)


@functools.lru_cache(maxsize=None)
def _three_launch(rows, C, res, scale, params=True):
    """(dy, dx, dxs, dW1, db1, dgamma, dbeta) of the three launches of today."""
    from segmentation_factory_amd import hip
    t = _inputs(rows, C)
    dy = hip.gemm(1, t['dh'], t['w1'], rows, C, 4 * C)
    dx, dg, db = hip.layernorm_bwd(t['x'], dy, t['gamma'], t['mean'], t['rstd'], dres=t['dres'] if res else None,
                                   rscale=t['rscale'] if scale else None, rows_per_group=t['rpg'])
    dxs = dx.scaled
    dx.scaled = None
    if scale:
        assert dxs is not None and torch.equal(dxs, hip.scale_rows(dx, t['rscale'], t['rpg']))
    dw = db1 = None
    if params:
        dw, db1 = hip.gemm_dw_db(t['dh'], t['y'], 4 * C, C, rows, split_k=hip.pick_splitk(4 * C, C, rows))
    return dy, dx, dxs, dw, db1, dg, db


@functools.lru_cache(maxsize=None)
def _oracle(rows, C):
    """float64 (dW1, db1, dgamma, dbeta) from the bf16 inputs, the bf16-rounded dy and the saved fp32 row statistics."""
    t = _inputs(rows, C)
    dy = _three_launch(rows, C, False, False)[0].double()
    dh, y, x = t['dh'].double(), t['y'].double(), t['x'].double()
    xh = (x - t['mean'].double()[:, None]) * t['rstd'].double()[:, None]
    return dh.t() @ y, dh.sum(0), (dy * xh).sum(0), dy.sum(0)


def _check_params(tag, fused, three, oracle):
    ratios = {}
    for name, f, p, o in zip(('dW1', 'db1', 'dgamma', 'dbeta'), fused, three, oracle):
        ef, ep = (f.double() - o).abs().max().item(), (p.double() - o).abs().max().item()
        ratios[name] = (ef, ep)
        print(f'{tag} {name}: fused max err {ef:.3e}, three-launch max err {ep:.3e}, ratio {ef / ep if ep else float("inf"):.3f}')
    for name, (ef, ep) in ratios.items():
        assert ef <= 2.0 * ep, (tag, name, ef, ep)


@pytest.mark.parametrize('scale', [False, True], ids=['noscale', 'rscale'])
@pytest.mark.parametrize('res', [False, True], ids=['nores', 'dres'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_fused_entry_point_against_the_three_launches(shape, res, scale, monkeypatch):
    from segmentation_factory_amd import hip
    rows, C = shape
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '2')
    assert hip.layernorm_linear_bwd_supported(torch.bfloat16, rows, C, 4 * C)
    t = _inputs(rows, C)
    dy0, dx0, dxs0, dw0, db10, dg0, db0 = _three_launch(rows, C, res, scale)
    kw = dict(dres=t['dres'] if res else None, rscale=t['rscale'] if scale else None, rows_per_group=t['rpg'])
    with hip.trace() as tr:
        dx1, dw1, db11, dg1, db1, dy1 = hip.layernorm_linear_bwd(t['dh'], t['w1'], t['x'], t['y'], t['gamma'], t['mean'], t['rstd'],
                                                                 return_dy=True, **kw)
    assert tr.kernels[0].startswith(f'ln_linear_bwd_kernel<{C // 32}>') and len(tr.kernels) == 4, tr.kernels
    dxs1 = dx1.scaled
    # deferred finalize into one flat buffer laid out as the optimizer's gradient buffer lays the four parameters out
    N = 4 * C
    flat = torch.full((N * C + N + 2 * C,), float('nan'), device='cuda')
    outs = (flat[:N * C].view(N, C), flat[N * C:N * C + N], flat[N * C + N:N * C + N + C], flat[N * C + N + C:])
    dx2, items = hip.layernorm_linear_bwd(t['dh'], t['w1'], t['x'], t['y'], t['gamma'], t['mean'], t['rstd'], outs=outs, defer=True, **kw)
    dxs2 = dx2.scaled
    hip.colreduce_finalize_grouped(items)
    torch.cuda.synchronize()
    tag = f'({rows}, {C}) res={res} scale={scale}'
    for name, got, want in (('dy', dy1, dy0), ('dx', dx1, dx0), ('dx deferred', dx2, dx0)) + \
            ((('dxs', dxs1, dxs0), ('dxs deferred', dxs2, dxs0)) if scale else ()):
        print(f'{tag} {name}: unequal elements {(got != want).sum().item()} of {got.numel()}')
    assert torch.equal(dy1, dy0) and torch.equal(dx1, dx0) and torch.equal(dx2, dx0)
    if scale:
        assert torch.equal(dxs1, dxs0) and torch.equal(dxs2, dxs0)
        lo, hi = t['rpg'], min(2 * t['rpg'], rows)
        assert not dxs1[lo:hi].any() and dx1[lo:hi].any()             # the dropped sample
    else:
        assert dxs1 is None and dxs2 is None
    # the deferred sums are the immediate ones, and the kernel's partials do not depend on the run
    for a, b in zip(outs, (dw1, db11, dg1, db1)):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
    again = hip.layernorm_linear_bwd(t['dh'], t['w1'], t['x'], t['y'], t['gamma'], t['mean'], t['rstd'], **kw)
    for a, b in zip(again[1:], (dw1, db11, dg1, db1)):
        assert torch.equal(a, b)
    _check_params(tag, (dw1, db11, dg1, db1), (dw0, db10, dg0, db0), _oracle(rows, C))


@pytest.mark.parametrize('shape', THRESHOLDS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_data_gradient_follows_the_kernel_segf_gemm_takes_at_the_size(shape, monkeypatch):
    """From these row counts on segf_gemm forms fc1's data gradient on the streaming kernels; the C = 64 probe rows (see
    tests/test_ln_linear_bwd_cpu.py) tell the K-quarter order from every other."""
    from segmentation_factory_amd import hip
    from test_ln_linear_bwd_cpu import k_quarter_dy, order_probe
    rows, C = shape
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '2')
    t = _inputs(rows, C)
    if C == 64:
        dh_row, w_probe = order_probe()
        # (the probe's weights replace three columns of W1 for this case only; the shared inputs are restored below)
        saved_w, saved_dh = t['w1'][:, :3].clone(), t['dh'][rows - 1].clone()
        t['w1'][:, :3] = torch.from_numpy(w_probe[:, :3]).to(torch.bfloat16).cuda()
        t['dh'][rows - 1] = torch.from_numpy(dh_row).to(torch.bfloat16).cuda()
    try:
        with hip.trace() as tr:
            dy0 = hip.gemm(1, t['dh'], t['w1'], rows, C, 4 * C)
        assert tr.kernels[0].startswith('gemm_skinny_kernel<LAYOUT, 4, 2>' if C == 32 else 'gemm_skinny_k_kernel<LAYOUT, 2, NT>'), tr.kernels
        dx0, _, _ = hip.layernorm_bwd(t['x'], dy0, t['gamma'], t['mean'], t['rstd'], dres=t['dres'], rscale=t['rscale'], rows_per_group=t['rpg'])
        dx1, _, _, _, _, dy1 = hip.layernorm_linear_bwd(t['dh'], t['w1'], t['x'], t['y'], t['gamma'], t['mean'], t['rstd'], dres=t['dres'],
                                                        rscale=t['rscale'], rows_per_group=t['rpg'], return_dy=True)
        torch.cuda.synchronize()
        print(f'({rows}, {C}): dy unequal {(dy1 != dy0).sum().item()}, dx unequal {(dx1 != dx0).sum().item()}, '
              f'dxs unequal {(dx1.scaled != dx0.scaled).sum().item()} of {dx0.numel()}')
        assert torch.equal(dy1, dy0) and torch.equal(dx1, dx0) and torch.equal(dx1.scaled, dx0.scaled)
        if C == 64:
            want = torch.from_numpy(k_quarter_dy(dh_row, w_probe)[:3])
            assert torch.equal(dy1[rows - 1, :3].float().cpu(), want) and want.tolist() == [1.0, 0.0, 2.0]
    finally:
        if C == 64:
            t['w1'][:, :3], t['dh'][rows - 1] = saved_w, saved_dh


@pytest.mark.parametrize('dim,heads', [(32, 1), (64, 2)])
def test_mit_block_with_and_without_the_fused_backward(dim, heads, monkeypatch):
    """One MiT Block on an 18 x 30 map (batch 2, DropPath scales given, one sample dropped in the attention branch) under
    SEGFAC_LN_LINEAR_BWD_FUSED=2 and =0: output and input gradient bit-equal, every parameter gradient but the four of norm2 / fc1
    bit-equal, and those four within the bound of the kernel test against the float64 oracle of the fused call's own operands."""
    from segmentation_factory_amd import dispatch, functional as Fh, hip
    from segmentation_factory_amd.backbones import Block
    torch.manual_seed(5)
    B, H, W = 2, 18, 30
    blk = Block(dim, heads, sr_ratio=1, dpr=0.1).cuda()
    x0 = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    dy = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    s1 = torch.tensor([0.0, 1.0 / 0.9], device='cuda')
    s2 = torch.tensor([1.0 / 0.9, 1.0 / 0.9], device='cuda')
    captured = []
    real = hip.layernorm_linear_bwd

    def spy(*a, **k):
        captured.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(hip, 'layernorm_linear_bwd', spy)
    outs, fused_calls = [], []
    for pol in ('2', '0'):
        monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', pol)
        x = x0.clone().requires_grad_()
        for p in blk.parameters():
            p.grad = None
        with dispatch.record() as calls:
            y = blk.tokens(x, B, H, W, (s1, s2))
            y.backward(dy)
        torch.cuda.synchronize()
        fused_calls.append(sum(c['fn'] == 'segf_layernorm_linear_bwd' for c in calls))
        outs.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    assert fused_calls == [1, 0] and len(captured) == 1, fused_calls
    assert torch.equal(outs[0][0], outs[1][0])
    print(f'dim {dim}: input gradient unequal elements {(outs[0][1] != outs[1][1]).sum().item()} of {outs[0][1].numel()}')
    assert torch.equal(outs[0][1], outs[1][1])
    four = ('mlp.fc1.weight', 'mlp.fc1.bias', 'norm2.weight', 'norm2.bias')
    assert set(outs[0][2]) == set(outs[1][2]) and len(outs[0][2]) >= 16 and all(k in outs[0][2] for k in four)
    for k, gnew in outs[0][2].items():
        if k not in four:
            assert torch.equal(gnew, outs[1][2][k]), k
    (dh, w1, xin, yin, gamma, mean, rstd), kw = captured[0]
    assert kw.get('rscale') is not None and kw.get('dres') is not None          # the DropPath hand-over and the residual gradient are in play
    dyb = hip.gemm(1, dh, w1, dh.shape[0], dim, 4 * dim).double()
    xh = (xin.double() - mean.double()[:, None]) * rstd.double()[:, None]
    oracle = (dh.double().t() @ yin.double(), dh.double().sum(0), (dyb * xh).sum(0), dyb.sum(0))
    _check_params(f'Block dim {dim}', [outs[0][2][k].reshape(o.shape) for k, o in zip(four, oracle)],
                  [outs[1][2][k].reshape(o.shape) for k, o in zip(four, oracle)], oracle)
    assert Fh._SCALED_DY == {}                                                  # the parked scaled gradient was collected
