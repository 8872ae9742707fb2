"""ConvFormer (MetaFormer) on the GPU: the StarReLU and residual-scale kernels (csrc/metaformer.hip) against their float64 restatement
(tests/metaformer_refs.py, pinned to the reference by tests/test_convformer_cpu.py), convformer_s18 + SegFormerHead against the reference's
captured values (tests/golden/e2e_convformer_s18_*, tools/make_convformer_goldens.py), and the captured train step."""
import functools
import os

import numpy as np
import pytest
import torch

import metaformer_refs as R
from test_convformer_cpu import FIXTURES, NEVER_RUN, SCALE_SHAPES, SCALE_SLICE, STAR_SHAPES, STAR_SLICE
from test_kernels_gpu import _close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SUM_RT = 2 * 2e-5          # the fp32 sums: the project's factor-2 convention for row sums, on the float64 sum of the absolute terms


def _sum_close(got, ref, terms, what):
    """An fp32 sum against float64: |error| <= 2 x 2e-5 x sum |terms| (both dtypes accumulate in fp32: one bar)."""
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    err = (got.detach().double().cpu() - ref).abs()
    bar = SUM_RT * terms
    print(f'  {what}: max err {err.max().item():.3e}, smallest bar {float(torch.as_tensor(bar).min()):.3e}')
    assert bool((err <= bar).all()), f'{what}: err {err.max().item():.3e} vs bar {bar}'


@functools.lru_cache(maxsize=None)
def _star_case(shape, dtype):
    """Inputs rounded to the storage dtype (fp32 tensors) and the float64 references of one shape; computed once, never modified."""
    rows, cols = shape
    gen = torch.Generator().manual_seed(3000 + rows + cols)
    u = torch.randn(rows, cols, generator=gen).to(dtype).float()
    dy = torch.randn(rows, cols, generator=gen).to(dtype).float()
    u[::5, ::3] = 0.0                                                   # exact zeros among the inputs
    s, b = torch.tensor([1.17]), torch.tensor([-0.23])
    ud, dyd, sd, bd = u.double(), dy.double(), s.double(), b.double()
    ref = {'y': R.starrelu_fwd(ud, sd, bd)}
    ref['du'], ref['ds'], ref['db'] = R.starrelu_bwd(dyd, ud, sd)
    ref['ds_terms'], ref['db_terms'] = R.starrelu_sum_terms(dyd, ud)
    return {'u': u, 'dy': dy, 's': s, 'b': b}, ref


@functools.lru_cache(maxsize=None)
def _scale_case(shape, dtype):
    rows, C = shape
    gen = torch.Generator().manual_seed(4000 + rows + C)
    x = torch.randn(rows, C, generator=gen).to(dtype).float()
    dy = torch.randn(rows, C, generator=gen).to(dtype).float()
    scale = 1.0 + 0.1 * torch.randn(C, generator=gen)
    ref = {'y': R.colscale_fwd(x.double(), scale.double())}
    ref['dx'], ref['dscale'] = R.colscale_bwd(dy.double(), x.double(), scale.double())
    ref['dscale_terms'] = (dy.double() * x.double()).abs().sum(0)
    return {'x': x, 'dy': dy, 'scale': scale}, ref


def _dev(i, dtype):
    return {k: (v.cuda().to(dtype) if k in ('u', 'x', 'dy') else v.cuda()) for k, v in i.items()}


def _run_star(t):
    from segmentation_factory_amd import hip
    o = {'y': hip.starrelu_fwd(t['u'], t['s'], t['b'])}
    o['du'], o['ds'], o['db'] = hip.starrelu_bwd(t['u'], t['dy'], t['s'])
    torch.cuda.synchronize()
    return o


def _run_scale(t):
    from segmentation_factory_amd import hip
    o = {'y': hip.colscale_fwd(t['x'], t['scale'])}
    o['dx'], o['dscale'] = hip.colscale_bwd(t['dy'], t['x'], t['scale'])
    torch.cuda.synchronize()
    return o


def _check_star(o, ref, dtype):
    assert o['y'].dtype == o['du'].dtype == dtype
    _close(o['y'], ref['y'], dtype)
    _close(o['du'], ref['du'], dtype)
    _sum_close(o['ds'], ref['ds'], ref['ds_terms'], 'ds')
    _sum_close(o['db'], ref['db'], ref['db_terms'], 'db')


def _check_scale(o, ref, dtype):
    assert o['y'].dtype == o['dx'].dtype == dtype
    _close(o['y'], ref['y'], dtype)
    _close(o['dx'], ref['dx'], dtype)
    _sum_close(o['dscale'], ref['dscale'], ref['dscale_terms'], 'dscale')


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', STAR_SHAPES, ids=str)
def test_starrelu_kernel_parity(shape, dtype):
    """StarReLU forward and backward, called directly and through the autograd Function (same bits), against float64."""
    from segmentation_factory_amd import functional as Fh, hip
    i, ref = _star_case(shape, dtype)
    t = _dev(i, dtype)
    nblk = hip.lib().segf_starrelu_blocks(*shape)
    assert (nblk == 1) if shape == (12, 128) else (nblk > 1)               # one workgroup; several partial sums
    if shape == (1320, 1280):
        assert nblk == 105
    with hip.trace() as tr:
        o = _run_star(t)
    for name in ('starrelu_fwd_kernel', 'starrelu_bwd_kernel', 'starrelu_finalize_kernel'):
        assert any(name in k for k in tr.kernels), (name, tr.kernels)
    _check_star(o, ref, dtype)
    # exact zeros in u: zero gradient
    assert not bool(o['du'][::5, ::3].float().abs().sum().item())
    u = t['u'].clone().requires_grad_(True)
    s, b = t['s'].clone().requires_grad_(True), t['b'].clone().requires_grad_(True)
    y = Fh.star_relu(u, s, b)
    y.backward(t['dy'])
    assert torch.equal(y, o['y']) and torch.equal(u.grad, o['du']) and torch.equal(s.grad, o['ds']) and torch.equal(b.grad, o['db'])


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SCALE_SHAPES, ids=str)
def test_colscale_kernel_parity(shape, dtype):
    """The residual scale forward and backward, called directly and through the autograd Function (same bits), against float64."""
    from segmentation_factory_amd import functional as Fh, hip
    i, ref = _scale_case(shape, dtype)
    t = _dev(i, dtype)
    if shape == (2640, 512):
        assert hip.lib().segf_colscale_blocks(*shape) > 1
    with hip.trace() as tr:
        o = _run_scale(t)
    for name in ('colscale_fwd_kernel', 'colscale_bwd_kernel', 'colreduce_finalize_kernel'):
        assert any(name in k for k in tr.kernels), (name, tr.kernels)
    _check_scale(o, ref, dtype)
    x = t['x'].clone().requires_grad_(True)
    sc = t['scale'].clone().requires_grad_(True)
    y = Fh.col_scale(x, sc)
    y.backward(t['dy'])
    assert torch.equal(y, o['y']) and torch.equal(x.grad, o['dx']) and torch.equal(sc.grad, o['dscale'])


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_backward_is_reproducible(dtype):
    for shape, case, run in ((STAR_SHAPES[3], _star_case, _run_star), (STAR_SHAPES[2], _star_case, _run_star),
                             (SCALE_SHAPES[3], _scale_case, _run_scale), (SCALE_SHAPES[2], _scale_case, _run_scale)):
        t = _dev(case(shape, dtype)[0], dtype)
        a, b = run(t), run(t)
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_starrelu_edge_inputs(dtype):
    """u all negative: y == b exactly, du == 0, ds == 0.  (Exact zeros inside a random u: test_starrelu_kernel_parity.)"""
    from segmentation_factory_amd import hip
    i, _ = _star_case(STAR_SHAPES[1], dtype)
    t = _dev(i, dtype)
    u = -(t['u'].float().abs() + 0.5).to(dtype)
    y = hip.starrelu_fwd(u, t['s'], t['b'])
    du, ds, db = hip.starrelu_bwd(u, t['dy'], t['s'])
    assert torch.equal(y, t['b'].to(dtype).expand_as(y))
    assert not bool(du.float().abs().sum().item()) and float(ds.item()) == 0.0
    _sum_close(db, i['dy'].double().sum().reshape(1), i['dy'].double().abs().sum().item(), 'db')


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_kernels_read_and_write_column_slices(dtype):
    """Operands as column slices of a 3x-wide buffer give the bits of the contiguous call, and the sentinel columns beside the written
    slices are untouched."""
    from segmentation_factory_amd import hip
    rows, cols = STAR_SLICE
    t = _dev(_star_case(STAR_SLICE, dtype)[0], dtype)
    o = _run_star(t)
    wide = torch.full((rows, 3 * cols), 7.0, dtype=dtype, device='cuda')
    wide[:, cols:2 * cols] = t['u']
    gw = torch.full((rows, 3 * cols), 7.0, dtype=dtype, device='cuda')
    gw[:, :cols] = t['dy']
    out = torch.full((rows, 3 * cols), -3.0, dtype=dtype, device='cuda')
    y = hip.starrelu_fwd(wide[:, cols:2 * cols], t['s'], t['b'], y=out[:, 2 * cols:])
    assert torch.equal(y, o['y']) and y.data_ptr() == out[:, 2 * cols:].data_ptr()
    assert bool((out[:, :2 * cols] == -3.0).all())
    du, ds, db = hip.starrelu_bwd(wide[:, cols:2 * cols], gw[:, :cols], t['s'], du=out[:, cols:2 * cols])
    assert torch.equal(du, o['du']) and torch.equal(ds, o['ds']) and torch.equal(db, o['db'])
    assert bool((out[:, :cols] == -3.0).all()) and torch.equal(out[:, 2 * cols:], o['y'])
    assert bool((wide[:, :cols] == 7.0).all()) and bool((wide[:, 2 * cols:] == 7.0).all()) and bool((gw[:, cols:] == 7.0).all())

    rows, C = SCALE_SLICE
    t = _dev(_scale_case(SCALE_SLICE, dtype)[0], dtype)
    o = _run_scale(t)
    _check_scale(o, _scale_case(SCALE_SLICE, dtype)[1], dtype)
    wide = torch.full((rows, 3 * C), 7.0, dtype=dtype, device='cuda')
    wide[:, 2 * C:] = t['x']
    gw = torch.full((rows, 3 * C), 7.0, dtype=dtype, device='cuda')
    gw[:, C:2 * C] = t['dy']
    out = torch.full((rows, 3 * C), -3.0, dtype=dtype, device='cuda')
    y = hip.colscale_fwd(wide[:, 2 * C:], t['scale'], y=out[:, :C])
    assert torch.equal(y, o['y']) and bool((out[:, C:] == -3.0).all())
    dx, dscale = hip.colscale_bwd(gw[:, C:2 * C], wide[:, 2 * C:], t['scale'], dx=out[:, C:2 * C])
    assert torch.equal(dx, o['dx']) and torch.equal(dscale, o['dscale'])
    assert torch.equal(out[:, :C], o['y']) and bool((out[:, 2 * C:] == -3.0).all())
    assert bool((wide[:, :2 * C] == 7.0).all()) and bool((gw[:, :C] == 7.0).all()) and bool((gw[:, 2 * C:] == 7.0).all())


def test_unsupported_width_is_refused_before_any_launch():
    """cols = 220: an exception that names the shape, raised before any launch; the raw entry points return SEGF_ERR_SHAPE."""
    from segmentation_factory_amd import functional as Fh, hip
    x = torch.randn(70, 220, device='cuda')
    one = torch.ones(1, device='cuda')
    with hip.trace() as t:
        with pytest.raises(RuntimeError, match=r'70 rows of 220 columns'):
            Fh.star_relu(x, one, one)
        with pytest.raises(RuntimeError, match=r'70 rows of 220 columns'):
            Fh.col_scale(x, torch.ones(220, device='cuda'))
        p = x.data_ptr()
        assert hip.lib().segf_starrelu_fwd(0, 70, 220, p, 220, p, p, p, 220, None) == hip.ERR_SHAPE
        assert hip.lib().segf_colscale_fwd(0, 70, 220, p, 220, p, p, 220, None) == hip.ERR_SHAPE
    assert t.kernels == []
    torch.cuda.synchronize()


# ---- model parity -------------------------------------------------------------------------------------------------------------------------
# Gradient bars (fraction of a parameter's gradient scale, the convention of tests/test_crossformer_gpu.py::CROSSFORMER_GRAD_RT): twice
# the worst sample error / scale the test printed at its first MI355X run against the fixtures; the fp32 bar may not exceed 1e-3.
# Measured: fp32 6.00e-5 (96x128, backbone.stages.2.1.mlp.act.scale) and 6.43e-5 (72x104, backbone.stages.1.0.token_mixer.act1.bias);
# bf16 8.42e-1 (96x128, backbone.stages.2.1.mlp.act.scale) and 4.19e-1 (72x104, backbone.stages.1.1.token_mixer.act1.bias).  The worst
# gradient-norm errors, held to the same bars, were 1.5e-5 (fp32) and 1.7e-1 (bf16).  Every worst case is a one-element StarReLU
# parameter: its gradient is one signed sum over a whole activation tensor (2 x 10^4 to 6 x 10^5 terms here) that cancels to a small
# remainder, so in bf16 the storage rounding of dy and u (2^-9 per term, fp32 accumulation on both sides) is of the size of the sum itself;
# the fp32 figures show that the arithmetic is the reference's.  The test prints the worst figure of the parameters with more than one
# element beside it: 8.7e-6 (fp32) and 1.13e-1 (bf16, backbone.stages.2.4.res_scale1.scale) at that run.
CONVFORMER_GRAD_RT = {torch.float32: 1.29e-4, torch.bfloat16: 1.69}


def _fixture_model(golden_dir, fixture, dtype):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_convformer_goldens import convformer_state_dict, load_inventory
    g = np.load(os.path.join(golden_dir, fixture))
    sd = convformer_state_dict(load_inventory(g), int(g['weight_seed']))
    norms = [sd[str(k)].double().norm().item() for k in g['keys']]
    assert np.allclose(norms, g['weight_norms'], rtol=1e-12, atol=0), 'the weights are not the ones the fixture was made with'
    m = SegmentationModel(str(g['backbone']), num_classes=int(g['nc']), seg_head=str(g['head']), compute_dtype=dtype)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    m.decode_head.dropout.p = 0.0
    return g, m.cuda()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('fixture', FIXTURES, ids=['96x128', '72x104'])
def test_convformer_s18_against_reference_golden(golden_dir, fixture, dtype):
    """convformer_s18 + SegFormerHead, batch 2, against the reference's captured values: head output in eval and train mode, a strided
    sample of the full-size eval logits, loss, the head BatchNorm's running statistics after the first train-mode forward, sampled
    parameter gradients and gradient norms; the eight tensors of the unused classification tail receive no gradient."""
    from oracle import weights as OW
    from segmentation_factory_amd import criterion_lowres
    from tools.make_convformer_goldens import sample_indices
    g, model = _fixture_model(golden_dir, fixture, dtype)
    nc, B, H, W, seed = int(g['nc']), int(g['B']), int(g['H']), int(g['W']), int(g['seed'])
    x, y = OW.synthetic_batch(B, H, W, nc, seed)
    fp32 = dtype == torch.float32
    rel = 1e-3 if fp32 else 5e-2
    model.eval()
    with torch.no_grad():
        ev = model(x.cuda()).cpu().numpy()
        lo = model.forward_lowres(x.cuda()).nchw().float().cpu().numpy()
    assert lo.shape == g['lowres_eval'].shape == (B, nc, H // 4, W // 4)
    e_lo = np.abs(lo - g['lowres_eval']).max() / np.abs(g['lowres_eval']).max()
    e_ev = np.abs(ev[:, :, 1::8, 2::8] - g['logits_eval_sub']).max() / np.abs(g['logits_eval_sub']).max()
    print(f'  eval head output err/scale {e_lo:.3e}, full-size sample {e_ev:.3e} (bar {rel})')
    assert e_lo <= rel and e_ev <= rel
    model.train()
    lo = model.forward_lowres(x.cuda())
    loss = criterion_lowres(lo, y.cuda(), (H, W), None, num_classes=nc, dice=True, ignore_index=255)
    loss.backward()
    e_loss = abs(loss.item() - float(g['loss'])) / abs(float(g['loss']))
    print(f'  loss {loss.item():.6f} vs {float(g["loss"]):.6f}: rel {e_loss:.3e}')
    assert e_loss <= (2e-4 if fp32 else 2e-2)
    after = model.state_dict()
    for i, name in enumerate(g['bn_names']):
        name = str(name)
        assert int(after[f'{name}.num_batches_tracked']) == int(g['bn_num_batches_tracked'][i]) == 1, name
        for stat in ('running_mean', 'running_var'):
            ref = g[f'bn{i}_{stat}']
            err = np.abs(after[f'{name}.{stat}'].float().cpu().numpy() - ref).max() / np.abs(ref).max()
            print(f'  {name}.{stat}: err/scale {err:.3e}')
            if fp32:
                assert err <= 1e-5, (name, stat, err)
    with torch.no_grad():
        tr = model.forward_lowres(x.cuda()).nchw().float().cpu().numpy()        # second train-mode forward: same batch statistics
    e_tr = np.abs(tr - g['lowres_train']).max() / np.abs(g['lowres_train']).max()
    print(f'  train head output err/scale {e_tr:.3e} (bar {rel})')
    assert e_tr <= rel
    gmax = float(g['grad_global_max'])
    params = dict(model.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is None) == sorted(NEVER_RUN)
    rt = CONVFORMER_GRAD_RT[dtype]
    bad, worst, worst_norm, worst_many = [], (0.0, ''), (0.0, ''), (0.0, '')
    for i, name in enumerate(g['grad_names']):
        name = str(name)
        gr = params[name].grad
        ref_norm = float(g['grad_norms'][i])
        assert gr is not None, name
        gr = gr.detach().float().cpu()
        got = gr.flatten()[sample_indices(name, gr.numel())].numpy()
        norm = gr.double().norm().item()
        scale = np.abs(g['grad_samples'][i]).max() + ref_norm / max(1.0, np.sqrt(gr.numel())) + 1e-2 * gmax
        err = float(np.abs(got - g['grad_samples'][i]).max())
        nerr = abs(norm - ref_norm) / (ref_norm + 1e-1 * gmax)
        worst = max(worst, (err / scale, name))
        worst_norm = max(worst_norm, (nerr, name))
        if gr.numel() > 1:
            worst_many = max(worst_many, (err / scale, name))
        if err > rt * scale or nerr > rt:
            bad.append((name, err, rt * scale, norm, ref_norm))
    print(f'  worst gradient sample err/scale {worst[0]:.3e} ({worst[1]}); worst norm err {worst_norm[0]:.3e} ({worst_norm[1]}); '
          f'worst sample err/scale of the parameters with more than one element {worst_many[0]:.3e} ({worst_many[1]})')
    assert not bad, bad[:8]


def test_convformer_graphed_step(golden_dir, capsys):
    """Three steps of engine.train_one_epoch's default step (the captured hipGraph) with convformer_s18 + SegFormerHead, batch 2,
    72 x 104, 7 classes, fp32: one graph, finite losses, the first loss is the eager loss, and every parameter moves -- every StarReLU
    scale and bias and every residual scale included -- except the eight tensors of the unused classification tail, which ride on the
    optimizer's "received no gradient" flag."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from tools.make_convformer_goldens import convformer_state_dict, load_inventory
    g = np.load(os.path.join(golden_dir, FIXTURES[1]))
    nc, B, H, W, seed = 7, 2, 72, 104, 9
    sd = convformer_state_dict(load_inventory(g), 79)
    x, y = OW.learnable_batch(B, H, W, nc, seed)
    args = types.SimpleNamespace(nb_classes=nc, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)

    def build():
        m = SegmentationModel('convformer_s18', num_classes=nc, seg_head='SegFormerHead', compute_dtype=torch.float32)
        m.load_state_dict(sd, strict=True)
        m.decode_head.dropout.p = 0.0
        return m.cuda()

    eager = build().train()
    l_eager = criterion_lowres(eager.forward_lowres(x.cuda()), y.cuda(), (H, W), None, num_classes=nc, dice=True, ignore_index=255).item()
    model = build()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = FusedAGCAdamW(model.parameters(), lr=1e-3, weight_decay=0.0)       # no decay: a parameter moves only if its gradient arrived
    losses = []

    class Rec:
        def add_scalar(self, name, v, it=None):
            if name == 'train_loss':
                losses.append(float(v))
    engine.train_one_epoch(model, opt, [(x, y)] * 3, 0, 'cuda', 1, None, None, NativeScaler(), Rec(), args)
    out = capsys.readouterr().out
    assert getattr(model, '_graphed_step', None) is not None and out.count('captured as one hipGraph') == 1
    print(f'  graphed losses {losses}, eager first loss {l_eager:.7f}')
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert abs(losses[0] - l_eager) <= 1e-5 * max(1.0, abs(l_eager))
    still = sorted(k for k, v in model.named_parameters() if torch.equal(v.detach(), before[k]))
    assert still == sorted(NEVER_RUN), still[:12]
    assert sum(k.endswith(('.act1.scale', '.act1.bias', '.act.scale', '.act.bias')) for k in before) == 72
    assert sum('.res_scale' in k for k in before) == 24
    counts = {k: int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert len(counts) == 1 and set(counts.values()) == {3}
