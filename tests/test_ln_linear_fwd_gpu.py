"""`LayerNorm -> thin Linear` of MiT stages 1 / 2 without the stored LayerNorm output:

  A  segf_layernorm_linear_fwd (ln_linear_fwd_kernel) against segf_layernorm_fwd[_patch] + segf_gemm (layout 0): the product, mean, rstd,
     the patch-major copy and the optional token-order y are torch.equal
  B  segf_layernorm_linear_bwd_ex with y == NULL (y rebuilt from x) against segf_layernorm_linear_bwd with the stored y: EVERY output
     torch.equal, the four parameter gradients included (the same partial sums of the same bits)
  C  ... with N = C and the patch-major fan-in (norm1 -> q) against its three launches (segf_gemm layout 1, segf_gemm_dw_db,
     segf_layernorm_bwd_patch): dy, dx, dxs torch.equal; dWq, dbq, dgamma, dbeta are other summation orders -- both forms against a float64
     oracle on the same bf16 inputs, the fused form's largest error at most 2 x the three-launch form's own (the bound
     tests/test_ln_linear_bwd_gpu.py uses for the same kind of sums: both add the same products in fp32, in different trees)
  one MiT Block of each width under SEGFAC_LN_LINEAR_FWD_FUSED=2 against =0, eager and as a captured GraphedTrainStep.

The inputs mix norm_refs' LayerNorm input classes row by row (offsets, large and tiny scales, constant rows, outliers): the statistics have to
carry ln_fwd_kernel's bits on each of them."""
import functools

import pytest
import torch

from norm_refs import LN_CLASSES, make_x

pytestmark = pytest.mark.gpu

SHAPES = [(1620, 32), (1620, 64), (37, 32), (64, 64)]          # ragged last group / tile, several workgroups; one group; one tile
PATCH = {32: (2, 16, 32, 8), 64: (2, 16, 16, 4)}               # C -> (batch, H, W, sr): stage 1 / stage 2 geometry in small
EPS = 1e-5


def _mixed_x(rows, C, g):
    """[rows, C] bf16: row r takes input class LN_CLASSES[r % 6]"""
    parts = [make_x(cls, rows, C, g, 1) for cls in LN_CLASSES]
    x = torch.stack(parts, 0)[torch.arange(rows) % len(LN_CLASSES), torch.arange(rows)]
    return x.to(torch.bfloat16).cuda()


@functools.lru_cache(maxsize=None)
def _fwd_inputs(rows, C, N):
    g = torch.Generator().manual_seed(7000 * C + 10 * rows + N)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = _mixed_x(rows, C, g)
    gamma, beta = (1.0 + 0.3 * rn(C)).cuda(), (0.2 * rn(C)).cuda()
    w = (rn(N, C) * 0.2).to(torch.bfloat16).cuda()
    bias = (0.5 * rn(N)).cuda()
    return dict(x=x, gamma=gamma, beta=beta, w=w, bias=bias)


def _patch_index(B, H, W, sr, device='cuda'):
    """token row r -> its row in the patch-major order (csrc/norm.hip: patch_row), in integer arithmetic of its own"""
    r = torch.arange(B * H * W, device=device)
    b, yy, xx = r // (H * W), (r // W) % H, r % W
    return (((b * (H // sr) + yy // sr) * (W // sr) + xx // sr) * sr + yy % sr) * sr + xx % sr


def _nuneq(a, b):
    return (a != b).sum().item()


@pytest.mark.parametrize('wide', [1, 4], ids=['q', 'fc1'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_forward_against_the_two_launches(shape, wide, monkeypatch):
    from segmentation_factory_amd import hip
    rows, C = shape
    N = wide * C
    t = _fwd_inputs(rows, C, N)
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '0')
    assert not hip.layernorm_linear_fwd_supported(torch.bfloat16, rows, C, N)
    y0, mean0, rstd0 = hip.layernorm_fwd(t['x'], t['gamma'], t['beta'], EPS)
    out0 = hip.gemm(0, y0, t['w'], rows, N, C, bias=t['bias'])
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '2')
    assert hip.layernorm_linear_fwd_supported(torch.bfloat16, rows, C, N)
    with hip.trace() as tr:
        out1, mean1, rstd1, y1, col1 = hip.layernorm_linear_fwd(t['x'], t['gamma'], t['beta'], EPS, t['w'], t['bias'], keep_y=True)
    assert len(tr.kernels) == 1 and tr.kernels[0].startswith(f'ln_linear_fwd_kernel<{C // 32}, '), tr.kernels
    out2, mean2, rstd2, y2, _ = hip.layernorm_linear_fwd(t['x'], t['gamma'], t['beta'], EPS, t['w'], t['bias'])
    torch.cuda.synchronize()
    print(f'({rows}, {C}) -> {N}: unequal elements: out {_nuneq(out1, out0)} / {_nuneq(out2, out0)} of {out0.numel()}, mean {_nuneq(mean1, mean0)}, '
          f'rstd {_nuneq(rstd1, rstd0)} of {rows}, y {_nuneq(y1, y0)} of {y0.numel()}')
    assert col1 is None and y2 is None
    assert torch.isfinite(out0.float()).all()
    assert torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0) and torch.equal(y1, y0) and torch.equal(out1, out0)
    assert torch.equal(mean2, mean0) and torch.equal(rstd2, rstd0) and torch.equal(out2, out0)


@pytest.mark.parametrize('keep_y', [False, True], ids=['noy', 'y'])
@pytest.mark.parametrize('wide', [1, 4], ids=['q', 'fc1'])
@pytest.mark.parametrize('C', [32, 64])
def test_forward_patch_form_against_the_two_launches(C, wide, keep_y):
    from segmentation_factory_amd import hip
    B, H, W, sr = PATCH[C]
    rows, N = B * H * W, wide * C
    patch = (W.bit_length() - 1, sr.bit_length() - 1)
    t = _fwd_inputs(rows, C, N)
    y0, mean0, rstd0, col0 = hip.layernorm_fwd(t['x'], t['gamma'], t['beta'], EPS, patch=patch)
    out0 = hip.gemm(0, y0, t['w'], rows, N, C, bias=t['bias'])
    out1, mean1, rstd1, y1, col1 = hip.layernorm_linear_fwd(t['x'], t['gamma'], t['beta'], EPS, t['w'], t['bias'], patch=patch, keep_y=keep_y)
    torch.cuda.synchronize()
    print(f'patch C {C} -> {N}: unequal elements: out {_nuneq(out1, out0)}, col {_nuneq(col1, col0)} of {col0.numel()}')
    assert col1.shape == col0.shape == (rows // (sr * sr), sr * sr * C)
    # the patch-major copy is the token rows permuted (checked against index arithmetic of the test's own)
    assert torch.equal(col0.view(rows, C)[_patch_index(B, H, W, sr)], y0)
    assert torch.equal(col1, col0) and torch.equal(out1, out0) and torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0)
    assert (y1 is None) if not keep_y else torch.equal(y1, y0)


def test_default_policy_engages_from_131072_rows():
    """norm2 -> fc1 through functional.layer_norm_res_linear at 131072 x 32 under the default switches: ONE forward launch, no stored y, and the
    bits of the two launches that 131071 rows still take."""
    from segmentation_factory_amd import dispatch, functional as Fh, hip
    rows, C = 131072, 32
    assert hip.policy('ln_linear_fwd_fused') == 1 and hip.policy('ln_linear_bwd_fused') == 1
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(torch.bfloat16).cuda()
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(), (0.2 * torch.randn(C, generator=g)).cuda().requires_grad_()
    w, bias = (torch.randn(4 * C, C, generator=g) * 0.2).cuda().requires_grad_(), (0.5 * torch.randn(4 * C, generator=g)).cuda().requires_grad_()
    dh = torch.randn(rows, 4 * C, generator=g).to(torch.bfloat16).cuda()
    res = []
    for n in (rows, rows - 1):
        xi = x[:n].clone().requires_grad_()
        for p in (gamma, beta, w, bias):
            p.grad = None
        with dispatch.record() as calls:
            xo, h = Fh.layer_norm_res_linear(xi, gamma, beta, EPS, w, bias)
            torch.autograd.backward((xo, h), (torch.zeros_like(xo), dh[:n]))
        torch.cuda.synchronize()
        res.append(([c['fn'] for c in calls if c['fn'].startswith(('segf_layernorm', 'segf_gemm'))], h.detach(), xi.grad, w.grad.clone()))
    assert res[0][0] == ['segf_layernorm_linear_fwd', 'segf_layernorm_linear_bwd_ex'], res[0][0]
    assert res[1][0][:2] == ['segf_layernorm_fwd', 'segf_gemm'] and 'segf_layernorm_linear_fwd' not in res[1][0], res[1][0]
    print(f'default policy: h unequal {_nuneq(res[0][1][:rows - 1], res[1][1])}, dx unequal {_nuneq(res[0][2][:rows - 1], res[1][2])}')
    assert torch.equal(res[0][1][:rows - 1], res[1][1]) and torch.equal(res[0][2][:rows - 1], res[1][2])
    assert torch.isfinite(res[0][3]).all()


# ---- B: the backward of norm2 -> fc1 with y rebuilt from x ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_inputs(rows, C, N, groups=3):
    from segmentation_factory_amd import hip
    t = dict(_fwd_inputs(rows, C, N))
    g = torch.Generator().manual_seed(9000 * C + rows + N)
    t['dh'] = torch.randn(rows, N, generator=g).to(torch.bfloat16).cuda()
    t['dres'] = torch.randn(rows, C, generator=g).to(torch.bfloat16).cuda()
    t['dtok'] = torch.randn(rows, C, generator=g).to(torch.bfloat16).cuda()         # the second consumer's gradient, token order
    t['y'], t['mean'], t['rstd'] = hip.layernorm_fwd(t['x'], t['gamma'], t['beta'], EPS)
    t['rpg'] = (rows + groups - 1) // groups
    t['rscale'] = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9][:groups] if groups == 3 else [1.0 / 0.9, 0.0], device='cuda')      # one sample is dropped
    return t


def _flat_outs(N, C):
    flat = torch.full((N * C + N + 2 * C,), float('nan'), device='cuda')
    return flat[:N * C].view(N, C), flat[N * C:N * C + N], flat[N * C + N:N * C + N + C], flat[N * C + N + C:]


@pytest.mark.parametrize('scale', [False, True], ids=['noscale', 'rscale'])
@pytest.mark.parametrize('res', [False, True], ids=['nores', 'dres'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_backward_rebuilds_y_from_x(shape, res, scale):
    from segmentation_factory_amd import hip
    rows, C = shape
    N = 4 * C
    t = _bwd_inputs(rows, C, N)
    kw = dict(dres=t['dres'] if res else None, rscale=t['rscale'] if scale else None, rows_per_group=t['rpg'])
    args = (t['dh'], t['w'], t['x'])
    stats = (t['gamma'], t['mean'], t['rstd'])
    want = hip.layernorm_linear_bwd(*args, t['y'], *stats, return_dy=True, **kw)
    want_dxs = want[0].scaled
    with hip.trace() as tr:
        got = hip.layernorm_linear_bwd(*args, None, *stats, beta=t['beta'], return_dy=True, **kw)
    assert tr.kernels[0].startswith(f'ln_linear_bwd_kernel<{C // 32}, true, 4, false>') and len(tr.kernels) == 4, tr.kernels
    got_dxs = got[0].scaled
    outs = _flat_outs(N, C)
    dx2, items, dy2 = hip.layernorm_linear_bwd(*args, None, *stats, beta=t['beta'], outs=outs, defer=True, return_dy=True, **kw)
    dxs2 = dx2.scaled
    hip.colreduce_finalize_grouped(items)
    torch.cuda.synchronize()
    names = ('dx', 'dW1', 'db1', 'dgamma', 'dbeta', 'dy')
    tag = f'({rows}, {C}) res={res} scale={scale}'
    print(tag + ': unequal elements ' + ', '.join(f'{n} {_nuneq(a, b)}' for n, a, b in zip(names, got, want)))
    for n, a, b in zip(names, got, want):
        assert torch.equal(a, b), (tag, n)
    assert torch.equal(dx2, want[0]) and torch.equal(dy2, want[5])
    for n, a, b in zip(names[1:5], outs, want[1:5]):
        assert torch.equal(a.reshape(-1), b.reshape(-1)), (tag, n, 'deferred')
    if scale:
        assert torch.equal(got_dxs, want_dxs) and torch.equal(dxs2, want_dxs)
        lo, hi = t['rpg'], min(2 * t['rpg'], rows)
        assert not got_dxs[lo:hi].any() and got[0][lo:hi].any()               # the dropped sample
    else:
        assert got_dxs is None and dxs2 is None and want_dxs is None


# ---- C: the backward of norm1 -> q in one pass -------------------------------------------------------------------------------------
def _q_case(C, patch):
    """(inputs, rows, B, H, W, sr): the patch geometry of width C, or (1620, C) with the fan-in absent"""
    if patch:
        B, H, W, sr = PATCH[C]
        return _bwd_inputs(B * H * W, C, C, groups=2), B * H * W, B, H, W, sr
    return _bwd_inputs(1620, C, C), 1620, None, None, None, None


def _q_operands(C, patch):
    t, rows, B, H, W, sr = _q_case(C, patch)
    dcol = pgeom = None
    if patch:
        dcol = torch.empty_like(t['dtok'])
        dcol[_patch_index(B, H, W, sr)] = t['dtok']                              # the convolution's data gradient as its product leaves it
        dcol = dcol.view(rows // (sr * sr), sr * sr * C)
        pgeom = (W.bit_length() - 1, sr.bit_length() - 1)
    return t, rows, dcol, pgeom


@functools.lru_cache(maxsize=None)
def _q_three_launch(C, patch, res, scale):
    from segmentation_factory_amd import hip
    t, rows, dcol, pgeom = _q_operands(C, patch)
    dy = hip.gemm(1, t['dh'], t['w'], rows, C, C)
    dw, dbq = hip.gemm_dw_db(t['dh'], t['y'], C, C, rows, split_k=hip.pick_splitk(C, C, rows))
    dx, dg, db = hip.layernorm_bwd(t['x'], dy, t['gamma'], t['mean'], t['rstd'], dy2=dcol, dres=t['dres'] if res else None,
                                   rscale=t['rscale'] if scale else None, rows_per_group=t['rpg'], dy2_patch=pgeom)
    dxs = dx.scaled
    dx.scaled = None
    return dy, dx, dxs, dw, dbq, dg, db


@functools.lru_cache(maxsize=None)
def _q_oracle(C, patch):
    """float64 (dWq, dbq, dgamma, dbeta) from the bf16 inputs, the bf16-rounded dy (+ the fan-in) and the saved fp32 row statistics"""
    t, rows, dcol, pgeom = _q_operands(C, patch)
    dy = _q_three_launch(C, patch, False, False)[0].double()
    if patch:
        dy = dy + t['dtok'].double()
    dq, y, x = t['dh'].double(), t['y'].double(), t['x'].double()
    xh = (x - t['mean'].double()[:, None]) * t['rstd'].double()[:, None]
    return dq.t() @ y, dq.sum(0), (dy * xh).sum(0), dy.sum(0)


def _check_params(tag, fused, three, oracle, names=('dWq', 'dbq', 'dgamma', 'dbeta')):
    ratios = {}
    for name, f, p, o in zip(names, fused, three, oracle):
        ef, ep = (f.double() - o).abs().max().item(), (p.double() - o).abs().max().item()
        ratios[name] = (ef, ep)
        print(f'{tag} {name}: fused max err {ef:.3e}, three-launch max err {ep:.3e}, ratio {ef / ep if ep else float("inf"):.3f}')
    for name, (ef, ep) in ratios.items():
        assert ef <= 2.0 * ep, (tag, name, ef, ep)


@pytest.mark.parametrize('scale', [False, True], ids=['noscale', 'rscale'])
@pytest.mark.parametrize('res', [False, True], ids=['nores', 'dres'])
@pytest.mark.parametrize('patch', [True, False], ids=['patch', '1620'])
@pytest.mark.parametrize('C', [32, 64])
def test_q_backward_against_the_three_launches(C, patch, res, scale):
    from segmentation_factory_amd import hip
    t, rows, dcol, pgeom = _q_operands(C, patch)
    dy0, dx0, dxs0, dw0, dbq0, dg0, db0 = _q_three_launch(C, patch, res, scale)
    kw = dict(dres=t['dres'] if res else None, rscale=t['rscale'] if scale else None, rows_per_group=t['rpg'], beta=t['beta'], dy2=dcol,
              dy2_patch=pgeom)
    args = (t['dh'], t['w'], t['x'], None, t['gamma'], t['mean'], t['rstd'])
    with hip.trace() as tr:
        dx1, dw1, dbq1, dg1, db1, dy1 = hip.layernorm_linear_bwd(*args, return_dy=True, **kw)
    want = f'ln_linear_bwd_kernel<{C // 32}, true, 1, {"true" if patch else "false"}>'
    assert tr.kernels[0].startswith(want) and len(tr.kernels) == 4, tr.kernels
    dxs1 = dx1.scaled
    outs = _flat_outs(C, C)
    dx2, items = hip.layernorm_linear_bwd(*args, outs=outs, defer=True, **kw)
    dxs2 = dx2.scaled
    hip.colreduce_finalize_grouped(items)
    again = hip.layernorm_linear_bwd(*args, **kw)
    torch.cuda.synchronize()
    tag = f'q C={C} {"patch" if patch else "1620"} res={res} scale={scale}'
    print(f'{tag}: unequal elements dy {_nuneq(dy1, dy0)}, dx {_nuneq(dx1, dx0)} / deferred {_nuneq(dx2, dx0)} of {dx0.numel()}'
          + (f', dxs {_nuneq(dxs1, dxs0)}' if scale else ''))
    assert torch.equal(dy1, dy0) and torch.equal(dx1, dx0) and torch.equal(dx2, dx0)
    if scale:
        assert torch.equal(dxs1, dxs0) and torch.equal(dxs2, dxs0)
        lo, hi = t['rpg'], min(2 * t['rpg'], rows)
        assert not dxs1[lo:hi].any() and dx1[lo:hi].any()
    else:
        assert dxs1 is None and dxs2 is None
    # the deferred sums are the immediate ones, and two runs of the same call are bit-identical
    for a, b in zip(outs, (dw1, dbq1, dg1, db1)):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
    for a, b in zip(again, (dx1, dw1, dbq1, dg1, db1)):
        assert torch.equal(a, b)
    _check_params(tag, (dw1, dbq1, dg1, db1), (dw0, dbq0, dg0, db0), _q_oracle(C, patch))


# ---- one MiT Block of each width ----------------------------------------------------------------------------------------------------
FUSED_PARAMS = ('norm1.weight', 'norm1.bias', 'attn.q.weight', 'attn.q.bias', 'norm2.weight', 'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias')


def _block_case(dim):
    from segmentation_factory_amd.backbones import Block
    torch.manual_seed(5 + dim)
    B, H, W = 2, 16, 32
    sr = 8 if dim == 32 else 4
    blk = Block(dim, dim // 32, sr_ratio=sr, dpr=0.1).cuda()
    for p in blk.parameters():                                           # biases and norm offsets away from their zero initial values
        if p.ndim == 1:
            p.data.add_(0.1 * torch.randn_like(p))
    x0 = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    dy = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    s1 = torch.tensor([0.0, 1.0 / 0.9], device='cuda')
    s2 = torch.tensor([1.0 / 0.9, 1.0 / 0.9], device='cuda')
    return blk, x0, dy, (B, H, W), (s1, s2)


@pytest.mark.parametrize('dim', [32, 64])
def test_mit_block_with_and_without_the_fused_forms(dim, monkeypatch):
    """One MiT Block on a 16 x 32 map (sr 8 / 4, batch 2, DropPath scales given, one sample dropped in the attention branch) with both switches
    at 2 and at 0: output and input gradient bit-equal, every parameter gradient outside norm1 / q / norm2 / fc1 bit-equal (they are
    computed from data-path tensors alone: q, col, the hidden activation, dx of both norms), and those eight within the bound of the kernel
    tests against float64 oracles of the fused calls' own operands."""
    from segmentation_factory_amd import dispatch, functional as Fh, hip
    blk, x0, dy, (B, H, W), scales = _block_case(dim)
    captured = []
    real = hip.layernorm_linear_bwd

    def spy(*a, **k):
        captured.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(hip, 'layernorm_linear_bwd', spy)
    outs, fns = [], []
    for pol in ('2', '0'):
        monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', pol)
        monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', pol)
        x = x0.clone().requires_grad_()
        for p in blk.parameters():
            p.grad = None
        with dispatch.record() as calls:
            y = blk.tokens(x, B, H, W, scales)
            y.backward(dy)
        torch.cuda.synchronize()
        fns.append([c['fn'] for c in calls])
        outs.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    assert fns[0].count('segf_layernorm_linear_fwd') == 2 and fns[0].count('segf_layernorm_linear_bwd_ex') == 2, fns[0]
    assert 'segf_layernorm_fwd_patch' not in fns[0] and 'segf_layernorm_bwd_patch' in fns[1] and 'segf_layernorm_fwd_patch' in fns[1]
    assert not any(f.startswith('segf_layernorm_linear') for f in fns[1]), fns[1]
    assert len(captured) == 2
    print(f'dim {dim}: output unequal {_nuneq(outs[0][0], outs[1][0])}, input gradient unequal {_nuneq(outs[0][1], outs[1][1])} of {outs[0][1].numel()}')
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2]) and len(outs[0][2]) >= 16 and all(k in outs[0][2] for k in FUSED_PARAMS)
    for k, gnew in outs[0][2].items():
        if k not in FUSED_PARAMS:
            assert torch.equal(gnew, outs[1][2][k]), k
    # the oracles: the backward runs norm2 -> fc1 first, norm1 -> q second
    sr = blk.attn.sr_ratio
    for (a, kw), names in zip(captured, (FUSED_PARAMS[4:], FUSED_PARAMS[:4])):
        dh, w, xin, yin, gamma, mean, rstd = a
        assert yin is None and kw.get('beta') is not None and kw.get('dres') is not None
        N = w.shape[0]
        yst = hip.layernorm_fwd(xin, gamma, kw['beta'], blk.norm1.eps)[0].double()
        dyb = hip.gemm(1, dh, w, dh.shape[0], dim, N).double()
        if names[0] == 'norm1.weight':
            assert N == dim and kw.get('dy2') is not None and kw.get('dy2_patch') == (5, sr.bit_length() - 1) and kw.get('rscale') is None
            dyb = dyb + kw['dy2'].view(-1, dim)[_patch_index(B, H, W, sr)].double()
        else:
            assert N == 4 * dim and kw.get('dy2') is None and kw.get('rscale') is not None
        xh = (xin.double() - mean.double()[:, None]) * rstd.double()[:, None]
        oracle = ((dyb * xh).sum(0), dyb.sum(0), dh.double().t() @ yst, dh.double().sum(0))
        _check_params(f'Block dim {dim} {names[2][:-7]}', [outs[0][2][k].reshape(o.shape) for k, o in zip(names, oracle)],
                      [outs[1][2][k].reshape(o.shape) for k, o in zip(names, oracle)], oracle, names=names)
    assert Fh._SCALED_DY == {}                                                  # the parked scaled gradient was collected


@pytest.mark.parametrize('dim', [32, 64])
def test_mit_block_with_the_forward_switch_alone(dim, monkeypatch):
    """SEGFAC_LN_LINEAR_FWD_FUSED=2 with SEGFAC_LN_LINEAR_BWD_FUSED=0: norm1 -> q runs the one-pass forward with the token-order y as its
    optional output and the backward makes the three launches of before on it -- the very products of the unfused block, so EVERY gradient is
    bit-equal; norm2 -> fc1 stays on its separate formulas (its one formula is chosen by the backward switch)."""
    from segmentation_factory_amd import dispatch
    blk, x0, dy, (B, H, W), scales = _block_case(dim)
    outs, fns = [], []
    for pol in ('2', '0'):
        monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', pol)
        monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '0')
        x = x0.clone().requires_grad_()
        for p in blk.parameters():
            p.grad = None
        with dispatch.record() as calls:
            y = blk.tokens(x, B, H, W, scales)
            y.backward(dy)
        torch.cuda.synchronize()
        fns.append([c['fn'] for c in calls])
        outs.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    assert fns[0].count('segf_layernorm_linear_fwd') == 1 and 'segf_layernorm_fwd_patch' not in fns[0], fns[0]
    assert not any(f.startswith('segf_layernorm_linear_bwd') for f in fns[0]) and not any(f.startswith('segf_layernorm_linear') for f in fns[1])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2])
    for k, gnew in outs[0][2].items():
        assert torch.equal(gnew, outs[1][2][k]), k


class _BlockModel(torch.nn.Module):
    """A trainable LayerNorm in front of one Block (the Block's input then carries a gradient, as inside the backbone)"""

    def __init__(self, blk, dim, geom, scales):
        super().__init__()
        from segmentation_factory_amd.containers import LayerNormWeights
        self.pre, self.blk, self.geom, self.scales = LayerNormWeights(dim), blk, geom, scales

    def forward(self, x):
        from segmentation_factory_amd import functional as Fh
        x = Fh.layer_norm(x, self.pre.weight, self.pre.bias, self.pre.eps)
        return self.blk.tokens(x, *self.geom, self.scales)


@pytest.mark.parametrize('dim', [32, 64])
def test_graphed_train_step_of_a_block_replays_to_the_eager_result(dim, monkeypatch):
    """Three optimizer steps of the Block with both switches at 2, eager and as a captured GraphedTrainStep: the same loss curve (rtol 2e-5 as
    tests/test_model_gpu.py::test_graphed_step_matches_eager_step: the captured step sums the parameter gradients in the grouped launches'
    order), and the captured step does run the one-pass forms."""
    import copy
    import numpy as np
    from segmentation_factory_amd import hip
    from segmentation_factory_amd.graph import GraphedTrainStep
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler, param_groups_weight_decay
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '2')
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '2')
    blk, x0, dy, geom, scales = _block_case(dim)
    tgt = dy.float()
    calls = []
    real_f, real_b = hip.layernorm_linear_fwd, hip.layernorm_linear_bwd
    monkeypatch.setattr(hip, 'layernorm_linear_fwd', lambda *a, **k: (calls.append('f'), real_f(*a, **k))[1])
    monkeypatch.setattr(hip, 'layernorm_linear_bwd', lambda *a, **k: (calls.append('b'), real_b(*a, **k))[1])

    def loss_fn(model, x, t):
        return (model(x).float() * t).mean()

    curves = []
    for graphed in (False, True):
        model = _BlockModel(copy.deepcopy(blk), dim, geom, scales).cuda().train()
        opt = FusedAGCAdamW(param_groups_weight_decay(model, 0.025), lr=1e-2)
        losses = []
        del calls[:]
        if graphed:
            gs = GraphedTrainStep(model, opt, loss_fn, (x0, tgt), clip_grad=0.02, clip_mode='agc', warmup=1)
            for _ in range(3):
                losses.append(gs.step(x0, tgt).item())
        else:
            scaler = NativeScaler()
            for _ in range(3):
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(model, x0, tgt)
                losses.append(loss.item())
                scaler(loss, opt, clip_grad=0.02, clip_mode='agc', parameters=model.parameters())
        assert calls.count('f') >= 2 and calls.count('b') >= 2 and calls.count('f') == calls.count('b'), calls
        curves.append(losses)
    print(f'dim {dim}: eager {curves[0]}, graphed {curves[1]}')
    assert curves[0][0] != curves[0][-1]
    np.testing.assert_allclose(curves[1], curves[0], rtol=2e-5)
