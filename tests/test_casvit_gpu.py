"""CAS-ViT (RCViT) on the GPU: the three token-mixer kernel pairs (csrc/token_mixer.hip) against their float64 restatement
(tests/casvit_refs.py, pinned to the reference by tests/test_casvit_cpu.py), rcvit_s + SegFormerHead against the reference's captured
values (tests/golden/e2e_rcvit_s_*, tools/make_casvit_goldens.py), and the captured train step."""
import functools
import os

import numpy as np
import pytest
import torch

import casvit_refs as R
from test_casvit_cpu import KERNEL_SHAPES, SLICE_SHAPE, WIDE_SHAPE

ALL_SHAPES = KERNEL_SHAPES + [SLICE_SHAPE, WIDE_SHAPE]

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


# the bars of tests/test_kernels_gpu.py::_close
def _tol(dtype):
    return (2e-5, 2e-5) if dtype == torch.float32 else (3e-2, 3e-2)


def _close(got, ref, dtype, what, fac=1.0):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    rt, at = _tol(dtype)
    s = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f'  {what}: max err {err:.3e}, scale {s:.3e}, bar {fac * (rt * s + at * 1e-2):.3e}')
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert err <= fac * (rt * s + at * 1e-2), f'{what}: max err {err:.3e} vs scale {s:.3e} ({dtype})'


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs rounded to the storage dtype (fp32 tensors) and the float64 references of one shape; computed once, never modified."""
    B, H, W, C = shape
    M = B * H * W
    gen = torch.Generator().manual_seed(2000 + ALL_SHAPES.index(shape))

    def rnd(*s):
        return torch.randn(*s, generator=gen).to(dtype).float()
    i = {'x': rnd(M, C), 'r': torch.relu(rnd(M, C)), 'w': torch.randn(C, generator=gen) / C ** 0.5, 'dy': rnd(M, C),
         'dpool': torch.randn(B, C, generator=gen), 'k': rnd(M, C), 'gq': torch.sigmoid(torch.randn(B, C, generator=gen)),
         'gk': torch.sigmoid(torch.randn(B, C, generator=gen))}
    d = {k: v.double() for k, v in i.items()}
    ref = {}
    ref['y'], ref['s'], ref['pool'] = R.spatial_gate_fwd(d['x'], d['r'], d['w'], B)
    ref['dx'], ref['dr'], ref['dw'] = R.spatial_gate_bwd(d['dy'], d['dpool'], d['x'], d['r'], ref['s'], d['w'], B)
    ref['dx0'], _, ref['dw0'] = R.spatial_gate_bwd(d['dy'], None, d['x'], d['r'], ref['s'], d['w'], B)
    ref['u'] = R.channel_gate_mix_fwd(d['x'], d['k'], d['gq'], d['gk'])
    ref['dq1'], ref['dk1'], ref['dgq'], ref['dgk'] = R.channel_gate_mix_bwd(d['dy'], d['x'], d['k'], d['gq'], d['gk'])
    ref['z'] = R.gated_mul_fwd(d['x'], d['k'])
    ref['da'], ref['dv'] = R.gated_mul_bwd(d['dy'], d['x'], d['k'])
    return i, ref


def _dev(i, dtype):
    return {k: (v.cuda().to(dtype) if k in ('x', 'r', 'dy', 'k') else v.cuda()) for k, v in i.items()}


def _run_direct(t, shape):
    """Every kernel once through segmentation_factory_amd.hip; -> dict of outputs"""
    from segmentation_factory_amd import hip
    B, H, W, C = shape
    o = {}
    o['y'], o['s'], o['pool'] = hip.spatial_gate_fwd(t['x'], t['r'], t['w'], B, H * W)
    o['dx'], o['dr'], o['dw'] = hip.spatial_gate_bwd(t['dy'], t['dpool'], t['x'], t['r'], o['s'], t['w'], B, H * W)
    o['dx0'], _, o['dw0'] = hip.spatial_gate_bwd(t['dy'], None, t['x'], t['r'], o['s'], t['w'], B, H * W)
    o['u'] = hip.channel_gate_mix_fwd(t['x'], t['k'], t['gq'], t['gk'], B, H * W)
    o['dq1'], o['dk1'], o['dgq'], o['dgk'] = hip.channel_gate_mix_bwd(t['dy'], t['x'], t['k'], t['gq'], t['gk'], B, H * W)
    o['z'] = hip.gated_mul_fwd(t['x'], t['k'])
    o['da'], o['dv'] = hip.gated_mul_bwd(t['dy'], t['x'], t['k'])
    torch.cuda.synchronize()
    return o


FP32_SUMS = ('pool', 'dw', 'dw0', 'dgq', 'dgk')          # accumulated in fp32 over rows: fac = 2.0


def _check(o, ref, dtype, keys=None):
    for k in keys or ref:
        assert o[k].dtype == (torch.float32 if k in FP32_SUMS + ('s',) else dtype), k
        _close(o[k], ref[k], torch.float32 if k == 's' else dtype, k, fac=2.0 if k in FP32_SUMS else 1.0)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', KERNEL_SHAPES + [WIDE_SHAPE], ids=str)
def test_token_mixer_kernel_parity(shape, dtype):
    """The three kernel pairs, called directly and through their autograd Functions (same bits), against float64."""
    from segmentation_factory_amd import functional as Fh, hip
    B, H, W, C = shape
    i, ref = _case(shape, dtype)
    t = _dev(i, dtype)
    with hip.trace() as tr:
        o = _run_direct(t, shape)
    for name in ('spatial_gate_fwd_kernel', 'spatial_gate_bwd_kernel', 'channel_gate_mix_fwd_kernel', 'channel_gate_mix_bwd_kernel',
                 'gated_mul_fwd_kernel', 'gated_mul_bwd_kernel'):
        assert any(name in k for k in tr.kernels), (name, tr.kernels)
    _check(o, ref, dtype)
    # the autograd Functions
    x, r, k = (t[n].clone().requires_grad_(True) for n in ('x', 'r', 'k'))
    w4 = t['w'].view(1, C, 1, 1).clone().requires_grad_(True)
    y, pool = Fh.spatial_gate(x, r, w4, B, H * W)
    torch.autograd.backward([y, pool], [t['dy'], t['dpool']])
    assert torch.equal(y, o['y']) and torch.equal(pool, o['pool'])
    assert torch.equal(x.grad, o['dx']) and torch.equal(r.grad, o['dr']) and torch.equal(w4.grad.view(C), o['dw'])
    x.grad = None
    gq, gk = t['gq'].clone().requires_grad_(True), t['gk'].clone().requires_grad_(True)
    u = Fh.channel_gate_mix(x, k, gq, gk, B, H * W)
    u.backward(t['dy'])
    assert torch.equal(u, o['u']) and torch.equal(x.grad, o['dq1']) and torch.equal(k.grad, o['dk1'])
    assert torch.equal(gq.grad, o['dgq']) and torch.equal(gk.grad, o['dgk'])
    x.grad, k.grad = None, None
    z = Fh.gated_mul(x, k)
    z.backward(t['dy'])
    assert torch.equal(z, o['z']) and torch.equal(x.grad, o['da']) and torch.equal(k.grad, o['dv'])


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [KERNEL_SHAPES[3], KERNEL_SHAPES[2]], ids=str)
def test_token_mixer_backward_is_reproducible(shape, dtype):
    i, _ = _case(shape, dtype)
    t = _dev(i, dtype)
    a, b = _run_direct(t, shape), _run_direct(t, shape)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_token_mixer_reads_and_writes_column_slices(dtype):
    """x (and the operands in its place) as columns C .. 2C of a [M, 3C] buffer, its gradient into columns C .. 2C of another one that is
    filled with a sentinel: the same bits as the contiguous run, and the other columns stay untouched."""
    from segmentation_factory_amd import hip
    shape = SLICE_SHAPE
    B, H, W, C = shape
    M = B * H * W
    i, ref = _case(shape, dtype)
    t = _dev(i, dtype)
    o = _run_direct(t, shape)
    _check(o, ref, dtype)
    wide = torch.full((M, 3 * C), 7.0, dtype=dtype, device='cuda')
    wide[:, C:2 * C] = t['x']
    wide[:, 2 * C:] = t['k']
    xs, ks = wide[:, C:2 * C], wide[:, 2 * C:]
    assert xs.stride(0) == 3 * C

    def grad_buffer():
        return torch.full((M, 3 * C), -3.0, dtype=dtype, device='cuda')

    def untouched(buf, *cols):
        keep = torch.ones(3 * C, dtype=torch.bool)
        for c in cols:
            keep[c * C:(c + 1) * C] = False
        return bool((buf[:, keep.cuda()] == -3.0).all())
    y, s, pool = hip.spatial_gate_fwd(xs, t['r'], t['w'], B, H * W)
    assert torch.equal(y, o['y']) and torch.equal(s, o['s']) and torch.equal(pool, o['pool'])
    g = grad_buffer()
    dx, dr, dw = hip.spatial_gate_bwd(t['dy'], t['dpool'], xs, t['r'], s, t['w'], B, H * W, dx=g[:, C:2 * C])
    assert torch.equal(g[:, C:2 * C], o['dx']) and torch.equal(dr, o['dr']) and torch.equal(dw, o['dw']) and untouched(g, 1)
    assert torch.equal(hip.channel_gate_mix_fwd(xs, ks, t['gq'], t['gk'], B, H * W), o['u'])
    g = grad_buffer()
    _, _, dgq, dgk = hip.channel_gate_mix_bwd(t['dy'], xs, ks, t['gq'], t['gk'], B, H * W, dq1=g[:, C:2 * C], dk1=g[:, 2 * C:])
    assert torch.equal(g[:, C:2 * C], o['dq1']) and torch.equal(g[:, 2 * C:], o['dk1']) and untouched(g, 1, 2)
    assert torch.equal(dgq, o['dgq']) and torch.equal(dgk, o['dgk'])
    assert torch.equal(hip.gated_mul_fwd(xs, ks), o['z'])
    g = grad_buffer()
    hip.gated_mul_bwd(t['dy'], xs, ks, da=g[:, C:2 * C], dv=g[:, 2 * C:])
    assert torch.equal(g[:, C:2 * C], o['da']) and torch.equal(g[:, 2 * C:], o['dv']) and untouched(g, 1, 2)
    torch.cuda.synchronize()
    assert bool((wide[:, :C] == 7.0).all())


def test_width_outside_the_channel_rule_is_refused_on_the_host():
    """C = 220 (rcvit_xs's last stage): an exception that names the shape, raised before any launch; the raw entry points return
    SEGF_ERR_SHAPE."""
    from segmentation_factory_amd import functional as Fh, hip
    B, HW, C = 2, 12, 220
    x = torch.zeros(B * HW, C, device='cuda')
    g = torch.zeros(B, C, device='cuda')
    w = torch.zeros(1, C, 1, 1, device='cuda')
    with hip.trace() as t:
        with pytest.raises(RuntimeError, match=r'spatial gate: no kernel for 2 x 12 rows of 220 channels'):
            Fh.spatial_gate(x, x, w, B, HW)
        with pytest.raises(RuntimeError, match=r'channel gate mix: no kernel for 2 x 12 rows of 220 channels'):
            Fh.channel_gate_mix(x, x, g, g, B, HW)
        with pytest.raises(RuntimeError, match=r'gated product: no kernel for 1 x 24 rows of 220 channels'):
            Fh.gated_mul(x, x)
        lib, p = hip.lib(), x.data_ptr()
        assert lib.segf_spatial_gate_fwd(0, B, HW, C, p, C, p, p, p, p, C, p, p, None) == hip.ERR_SHAPE
        assert lib.segf_channel_gate_mix_fwd(0, B, HW, C, p, C, p, C, p, p, p, C, None) == hip.ERR_SHAPE
        assert lib.segf_gated_mul_fwd(0, B * HW, C, p, C, p, C, p, C, None) == hip.ERR_SHAPE
    assert t.kernels == []
    torch.cuda.synchronize()


def test_qkv_split3_is_the_three_column_blocks_of_one_product():
    """functional.qkv_split3: q, k, v equal the column blocks of the one [M, 3C] product to the GEMM's own rounding, and its backward equals
    the backward of that product fed with the gathered [dq | dk | dv] (fp32)."""
    from segmentation_factory_amd import functional as Fh
    torch.manual_seed(11)
    M, C = 234, 48
    x = torch.randn(M, C, device='cuda', requires_grad=True)
    w = (torch.randn(3 * C, C, 1, 1, device='cuda') / C ** 0.5).requires_grad_(True)
    d = [torch.randn(M, C, device='cuda') for _ in range(3)]
    q, k, v = Fh.qkv_split3(x, w)
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    torch.autograd.backward([q, k, v], d)
    xd, wd = x.detach().double().cpu(), w.detach().double().cpu().view(3 * C, C)
    full = xd @ wd.t()
    dcat = torch.cat(d, 1).double().cpu()
    _close(torch.cat([q, k, v], 1), full, torch.float32, 'qkv')
    _close(x.grad, dcat @ wd, torch.float32, 'dx', fac=2.0)
    _close(w.grad.view(3 * C, C), dcat.t() @ xd, torch.float32, 'dw', fac=2.0)


# ---- model parity -------------------------------------------------------------------------------------------------------------------------
# Gradient bars (fraction of a parameter's gradient scale, the convention of tests/test_crossformer_gpu.py::CROSSFORMER_GRAD_RT): twice
# the worst sample error / scale the test printed at its first MI355X run against the fixtures; the fp32 bar may not exceed 1e-3.
# Measured: fp32 3.19e-6 (128x160) and 9.36e-6 (72x104), both backbone.patch_embed.0.bias; bf16 6.94e-2 (128x160, patch_embed.4.bias)
# and 8.90e-2 (72x104, patch_embed.1.weight).  The worst gradient-norm errors, held to the same bars, were 6.4e-7 (fp32) and 1.6e-2
# (bf16).  (With a data seed that put one ReLU input 1e-6 from zero the fp32 figure was 2.0e-3 in one depthwise weight: a flipped
# mask, not arithmetic; tools/make_casvit_goldens.py now asserts a margin)
RCVIT_GRAD_RT = {torch.float32: 1.88e-5, torch.bfloat16: 0.178}
FIXTURES = ['e2e_rcvit_s_128x160.npz', 'e2e_rcvit_s_72x104.npz']


def _fixture_model(golden_dir, fixture, dtype):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_casvit_goldens import load_inventory, rcvit_state_dict
    g = np.load(os.path.join(golden_dir, fixture))
    sd = rcvit_state_dict(load_inventory(g), int(g['weight_seed']))
    norms = [sd[str(k)].double().norm().item() for k in g['keys']]
    assert np.allclose(norms, g['weight_norms'], rtol=1e-12, atol=0), 'the weights are not the ones the fixture was made with'
    m = SegmentationModel(str(g['backbone']), num_classes=int(g['nc']), seg_head=str(g['head']), compute_dtype=dtype)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    m.decode_head.dropout.p = 0.0
    return g, m.cuda()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('fixture', FIXTURES, ids=['128x160', '72x104'])
def test_rcvit_s_against_reference_golden(golden_dir, fixture, dtype):
    """rcvit_s + SegFormerHead, batch 2, against the reference's captured values: head output in eval and train mode, a strided sample of
    the full-size eval logits, loss, four BatchNorms' running statistics after the first train-mode forward, sampled parameter gradients
    and gradient norms."""
    from oracle import weights as OW
    from segmentation_factory_amd import criterion_lowres
    from tools.make_casvit_goldens import sample_indices
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
    # the running statistics after this ONE train-mode forward
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
    rt = RCVIT_GRAD_RT[dtype]
    bad, worst, worst_norm = [], (0.0, ''), (0.0, '')
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
        if err > rt * scale or nerr > rt:
            bad.append((name, err, rt * scale, norm, ref_norm))
    print(f'  worst gradient sample err/scale {worst[0]:.3e} ({worst[1]}); worst norm err {worst_norm[0]:.3e} ({worst_norm[1]})')
    assert not bad, bad[:8]


def test_rcvit_graphed_step(golden_dir, capsys):
    """Three steps of engine.train_one_epoch's default step (the captured hipGraph) with rcvit_s + SegFormerHead, batch 2, 72 x 104,
    7 classes, fp32: one graph, finite losses, the first loss is the eager loss, every parameter moves -- the channel-gate weights, whose
    gradients arrive through autograd from the kernels' gate gradients, included -- and every BatchNorm counts one batch per replay."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from tools.make_casvit_goldens import load_inventory, rcvit_state_dict
    g = np.load(os.path.join(golden_dir, FIXTURES[1]))
    nc, B, H, W, seed = 7, 2, 72, 104, 9
    sd = rcvit_state_dict(load_inventory(g), 78)
    x, y = OW.learnable_batch(B, H, W, nc, seed)
    args = types.SimpleNamespace(nb_classes=nc, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)

    def build():
        m = SegmentationModel('rcvit_s', num_classes=nc, seg_head='SegFormerHead', compute_dtype=torch.float32)
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
    assert getattr(model, '_graphed_step', None) is not None and 'captured as one hipGraph' in capsys.readouterr().out
    print(f'  graphed losses {losses}, eager first loss {l_eager:.7f}')
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert abs(losses[0] - l_eager) <= 1e-5 * max(1.0, abs(l_eager))
    moved = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert any('.attn.oper_k.1.block.1.' in k for k in before)
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:8]
    counts = {k: int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert len(counts) == 15 * 5 + 2 + 3 + 4 + 1 and set(counts.values()) == {3}, sorted(set(counts.values()))
