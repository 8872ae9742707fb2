"""CrossFormer on the GPU: the group-attention kernel pair (csrc/attention_group.hip) against a float64 CPU restatement built on
functional.group_token_index, crossformer_tiny + SegFormerHead against the reference's captured values (tests/golden/e2e_crossformer_tiny_*,
tools/make_crossformer_goldens.py), and the captured train step."""
import functools
import os

import numpy as np
import pytest
import torch

from test_crossformer_cpu import KERNEL_SHAPES, MULTI_GROUP_SHAPES

ALL_SHAPES = KERNEL_SHAPES + MULTI_GROUP_SHAPES

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SCALE = 32 ** -0.5


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
    assert err <= fac * (rt * s + at * 1e-2), f'{what}: max err {err:.3e} vs scale {s:.3e} ({dtype})'


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs rounded to the storage dtype and the float64 reference (o, dqkv, dbias) of one shape; computed once, never modified."""
    from segmentation_factory_amd import functional as Fh
    B, H, W, heads, G, I, lda = shape
    C, N, T = heads * 32, G * G, H * W
    gen = torch.Generator().manual_seed(1000 + ALL_SHAPES.index(shape))
    qkv = torch.randn(B * T, 3 * C, generator=gen).to(dtype).float()
    bias = (torch.randn(heads, N, N, generator=gen) * 0.5).float()
    do = torch.randn(B * T, C, generator=gen).to(dtype).float()
    idx = Fh.group_token_index(H, W, G, I, lda)
    idx = idx[(idx >= 0).any(1)]                                   # groups that are all padding compute nothing
    valid, safe = idx >= 0, idx.clamp(min=0)
    x = qkv.double().requires_grad_(True)
    bb = bias.double().requires_grad_(True)
    g = x.view(B, T, 3, heads, 32)[:, safe]                        # [B, groups, N, 3, heads, 32]
    q, k, v = (g[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))          # [B, groups, heads, N, 32]
    s = q @ k.transpose(-1, -2) * SCALE + bb[None, None]
    s = s.masked_fill(~valid[None, :, None, None, :], float('-inf'))             # padded keys
    o = (torch.softmax(s, -1) @ v).permute(0, 1, 3, 2, 4).reshape(B, idx.shape[0], N, C)
    out = torch.zeros(B, T, C, dtype=torch.float64)
    out[:, safe[valid]] = o[:, valid]                              # padded queries are cropped away
    out = out.view(B * T, C)
    (out * do.double()).sum().backward()
    return qkv, bias, do, out.detach(), x.grad.detach(), bb.grad.detach()


def _run(qkv, bias, do, shape, dtype):
    from segmentation_factory_amd import functional as Fh
    B, H, W, heads, G, I, lda = shape
    x = qkv.cuda().to(dtype).requires_grad_(True)
    b = bias.cuda().requires_grad_(True)
    o = Fh.group_attention(x, b, B, H, W, heads, G, I, lda)
    o.backward(do.cuda().to(dtype))
    torch.cuda.synchronize()
    return o.detach(), x.grad.detach(), b.grad.detach()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', ALL_SHAPES, ids=[str(s) for s in ALL_SHAPES])
def test_group_attention_kernel_parity(shape, dtype):
    """KERNEL_SHAPES: one group per backward workgroup.  MULTI_GROUP_SHAPES: two and three, so the running dbias sum, the reuse of the LDS
    tiles from group to group (with padding slots that differ between consecutive groups) and the slabs of workgroups past the first are
    held to the same bars (tests/test_crossformer_cpu.py::test_backward_workspace_counts_the_groups_per_workgroup pins the counts)."""
    from segmentation_factory_amd import hip
    qkv, bias, do, o_ref, dqkv_ref, dbias_ref = _case(shape, dtype)
    with hip.trace() as t:
        o, dqkv, dbias = _run(qkv, bias, do, shape, dtype)
        # (the trace is per thread and autograd runs the backward on its own: the same backward once more, called from here)
        B, H, W, heads, G, I, lda = shape
        x = qkv.cuda().to(dtype)
        lse = hip.group_attention_fwd(x, bias.cuda(), B, H, W, heads, G, I, lda, SCALE)[1]
        dqkv2, dbias2 = hip.group_attention_bwd(x, bias.cuda(), do.cuda().to(dtype), lse, B, H, W, heads, G, I, lda, SCALE)
    assert any('group_attn_fwd_kernel' in k for k in t.kernels) and any('group_attn_bwd_kernel' in k for k in t.kernels), t.kernels
    assert torch.equal(dqkv2, dqkv) and torch.equal(dbias2, dbias)
    assert o.dtype == dtype and dqkv.dtype == dtype and dbias.dtype == torch.float32
    _close(o, o_ref, dtype, 'o')
    _close(dqkv, dqkv_ref, dtype, 'dqkv')
    _close(dbias, dbias_ref, dtype, 'dbias', fac=2.0)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [KERNEL_SHAPES[2]] + MULTI_GROUP_SHAPES, ids=str)
def test_group_attention_backward_is_reproducible(shape, dtype):
    qkv, bias, do = _case(shape, dtype)[:3]
    a, b = _run(qkv, bias, do, shape, dtype), _run(qkv, bias, do, shape, dtype)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_group_attention_reads_a_column_slice(dtype):
    """qkv as columns 8 .. 8 + 3C of a wider buffer: the leading dimension is the buffer's."""
    from segmentation_factory_amd import functional as Fh
    shape = KERNEL_SHAPES[1]
    B, H, W, heads, G, I, lda = shape
    qkv, bias, do, o_ref, dqkv_ref, dbias_ref = _case(shape, dtype)
    C3 = qkv.shape[1]
    wide = torch.full((qkv.shape[0], C3 + 16), 7.0, dtype=dtype, device='cuda')
    wide[:, 8:8 + C3] = qkv.cuda().to(dtype)
    wide.requires_grad_(True)
    b = bias.cuda().requires_grad_(True)
    view = wide[:, 8:8 + C3]
    assert view.stride(0) == C3 + 16
    o = Fh.group_attention(view, b, B, H, W, heads, G, I, lda)
    o.backward(do.cuda().to(dtype))
    o2, dqkv2, dbias2 = _run(qkv, bias, do, shape, dtype)
    assert torch.equal(o.detach(), o2) and torch.equal(wide.grad[:, 8:8 + C3], dqkv2) and torch.equal(b.grad, dbias2)
    assert float(wide.grad[:, :8].abs().max()) == 0 and float(wide.grad[:, 8 + C3:].abs().max()) == 0
    _close(o, o_ref, dtype, 'o')


def test_group_larger_than_the_tile_is_refused_on_the_host():
    """A 9 x 3 map asks for one group of side 9 (81 tokens): an exception that names the shape, raised before any launch."""
    from segmentation_factory_amd import functional as Fh, hip
    heads = 2
    qkv = torch.zeros(27, 3 * 32 * heads, device='cuda')
    bias = torch.zeros(heads, 81, 81, device='cuda')
    with hip.trace() as t:
        with pytest.raises(RuntimeError, match=r'9 x 9 = 81 tokens.*9 x 3 map'):
            Fh.group_attention(qkv, bias, 1, 9, 3, heads, 9, 1, False)
    assert t.kernels == []
    lib = hip.lib()
    assert lib.segf_group_attention_fwd(0, 1, 9, 3, heads, 32, 9, 1, 0, qkv.data_ptr(), qkv.stride(0), bias.data_ptr(), 0.5, None, 64,
                                        None, None) == hip.ERR_SHAPE
    torch.cuda.synchronize()


# ---- model parity -------------------------------------------------------------------------------------------------------------------------
# Gradient bars (fraction of a parameter's gradient scale, as tests/test_model_gpu.py): twice the worst sample error / scale the test
# printed at its first MI355X run against the fixtures.  Measured: fp32 1.51e-5 (256x320, layers.0.downsample.reductions.0.bias) and
# 6.9e-6 (64x96); bf16 5.94e-2 (256x320, layers.1.blocks.0.attn.pos.pos_proj.bias) and 4.61e-2 (64x96).  The worst gradient-norm
# errors, held to the same bars, were 2.9e-6 (fp32) and 1.6e-2 (bf16).
CROSSFORMER_GRAD_RT = {torch.float32: 3e-5, torch.bfloat16: 0.12}
FIXTURES = ['e2e_crossformer_tiny_256x320.npz', 'e2e_crossformer_tiny_64x96.npz']


def _zero_stochastic(model):
    for mod in model.modules():
        if hasattr(mod, 'drop_prob'):
            mod.drop_prob = 0.0
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return model


def _fixture_model(golden_dir, fixture, dtype):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_crossformer_goldens import load_inventory, model_state_dict
    g = np.load(os.path.join(golden_dir, fixture))
    sd = model_state_dict(load_inventory(g), int(g['weight_seed']))
    norms = [sd[str(k)].double().norm().item() for k in g['keys']]
    assert np.allclose(norms, g['weight_norms'], rtol=1e-12, atol=0), 'the weights are not the ones the fixture was made with'
    m = SegmentationModel(str(g['backbone']), num_classes=int(g['nc']), seg_head=str(g['head']), compute_dtype=dtype)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return g, _zero_stochastic(m.cuda())


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('fixture', FIXTURES, ids=['256x320', '64x96'])
def test_crossformer_tiny_against_reference_golden(golden_dir, fixture, dtype):
    """crossformer_tiny + SegFormerHead, batch 2, against the reference's captured values: head output in eval and train mode, a strided
    sample of the full-size eval logits, loss, sampled parameter gradients and gradient norms."""
    from oracle import weights as OW
    from segmentation_factory_amd import criterion_lowres
    from tools.make_crossformer_goldens import sample_indices
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
    with torch.no_grad():
        tr = model.forward_lowres(x.cuda()).nchw().float().cpu().numpy()        # second train-mode forward: same batch statistics
    e_tr = np.abs(tr - g['lowres_train']).max() / np.abs(g['lowres_train']).max()
    print(f'  train head output err/scale {e_tr:.3e} (bar {rel})')
    assert e_tr <= rel
    gmax = float(g['grad_global_max'])
    params = dict(model.named_parameters())
    rt = CROSSFORMER_GRAD_RT[dtype]
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


def test_crossformer_graphed_step(golden_dir, capsys):
    """Three steps of engine.train_one_epoch's default step (the captured hipGraph) with crossformer_tiny + SegFormerHead, batch 2,
    64 x 96, 7 classes, fp32, stochastic rates 0: one graph, finite losses, the first loss is the eager loss, every parameter moves --
    the attn.pos.* ones, whose gradients arrive through autograd from the kernel's dbias, included."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from tools.make_crossformer_goldens import load_inventory, model_state_dict
    g = np.load(os.path.join(golden_dir, FIXTURES[1]))
    nc, B, H, W, seed = 7, 2, 64, 96, 9
    sd = model_state_dict(load_inventory(g), 77)
    x, y = OW.learnable_batch(B, H, W, nc, seed)
    args = types.SimpleNamespace(nb_classes=nc, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)

    def build():
        m = SegmentationModel('crossformer_tiny', num_classes=nc, seg_head='SegFormerHead', compute_dtype=torch.float32)
        m.load_state_dict(sd, strict=True)
        return _zero_stochastic(m.cuda())

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
    assert any('.attn.pos.' in k for k in before)
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:8]


def test_crossformer_drop_path_override():
    """The backbone's own drop-path plumbing on the GPU (fp32, batch 2, 64 x 96): with a keep mask that keeps sample 0 in every draw at
    scale 1 (keep = 1 - rate) and drops sample 1 in every draw, sample 0's features equal those of the model with all rates 0, and sample 1's
    do not (its blocks past the first pass x through)."""
    from oracle import weights as OW
    from segmentation_factory_amd import backbones
    torch.manual_seed(3)
    m = backbones.crossformer_tiny().cuda().train()
    m.compute_dtype = torch.float32
    x, _ = OW.synthetic_batch(2, 64, 96, 7, 5)
    rates = [r for b in m._blocks() for r in (b.drop_prob, b.drop_prob) if b.drop_prob > 0]
    keep = torch.zeros(len(rates), 2)
    keep[:, 0] = 1.0 - torch.tensor(rates)
    m.stochastic_override = {'drop_path': keep}
    with torch.no_grad():
        dropped = [t.data.view(2, -1).clone() for t in m.forward_tokens(x.cuda())]
        m.stochastic_override = None
        _zero_stochastic(m)
        plain = [t.data.view(2, -1) for t in m.forward_tokens(x.cuda())]
    for a, b in zip(dropped[2:], plain[2:]):
        s = b[0].abs().max().item()
        assert (a[0] - b[0]).abs().max().item() <= 2e-5 * s, 'sample 0 is kept at scale 1 in every draw'
        assert (a[1] - b[1]).abs().max().item() > 1e-2 * b[1].abs().max().item(), 'sample 1 is dropped in every draw'
