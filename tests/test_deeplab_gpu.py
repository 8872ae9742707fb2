"""GPU tests of the DeepLabV3 (ASPP) decode head: the dilated 3x3 convolution kernel (csrc/conv_dilated.hip) against F.conv2d on the
CPU, its tap culling against the all-taps form, elementwise dropout, the head against the reference's recorded values
(tests/golden/e2e_deeplabv3_mitb0_416x448.npz, made by tools/make_deeplab_goldens.py) and the graphed train step."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _close(got, ref, dtype, scale=None, fac=1.0):
    """tests/test_kernels_gpu.py::_close: 2e-5 of the largest element for fp32 storage, 3e-2 for bf16."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    rt = 2e-5 if dtype == torch.float32 else 3e-2
    s = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item()
    print(f'  err {err:.3e} scale {s:.3e} bar {fac * (rt * s + rt * 1e-2):.3e} ({dtype})')
    assert err <= fac * (rt * s + rt * 1e-2), f'max err {err:.3e} vs scale {s:.3e} ({dtype})'


def _q(t, dtype):
    return t.detach().to(dtype).float().clone()


# (B, H, W, Cin, Cout, d): the smallest shapes that reach each way the kernel can go wrong
DIL_SHAPES = [
    (1, 1, 1, 8, 8, 12),              # centre tap only, one pixel
    (2, 13, 14, 40, 24, 12),          # partial taps; K and N tails
    (2, 16, 16, 256, 256, 24),        # centre only: also a 1x1 conv
    (1, 40, 28, 72, 264, 36),         # vertical taps live, horizontal dead; Cout across an N tile
    (3, 37, 41, 320, 256, 12),        # pixel tiles that straddle image boundaries; MobileNetV2's width
    (2, 9, 11, 64, 32, 2),            # a small rate where every tap is live almost everywhere
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('cfg', DIL_SHAPES, ids=lambda c: 'x'.join(map(str, c)))
def test_dilated_conv3x3(cfg, dtype):
    """Forward, data gradient and weight gradient vs F.conv2d(padding=d, dilation=d) on inputs rounded to the storage dtype; the input
    is a column slice of a wider buffer; the weight gradient of a dead tap is exactly 0."""
    from segmentation_factory_amd import functional as Fh, hip
    B, H, W, I, O, d = cfg
    g = torch.Generator().manual_seed(60 + d)
    x = torch.randn(B, I, H, W, generator=g)
    w = torch.randn(O, I, 3, 3, generator=g) * (2.0 / (9 * I)) ** 0.5
    dy = torch.randn(B, O, H, W, generator=g)
    xr = _q(x, dtype).requires_grad_(True)
    wr = _q(w, dtype).requires_grad_(True)
    ref = F.conv2d(xr, wr, None, padding=d, dilation=d)
    ref.backward(_q(dy, dtype))
    tok = lambda t, c: t.permute(0, 2, 3, 1).reshape(B * H * W, c)   # noqa: E731
    buf = torch.zeros(B * H * W, I + 16, dtype=dtype, device='cuda')
    buf[:, 8:8 + I] = tok(x, I).to(dtype).cuda()
    xd = buf[:, 8:8 + I].detach().requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    with hip.trace() as t:
        y = Fh.conv3x3_dilated(xd, wd, B, H, W, d)
    assert any('conv3x3_dil_kernel' in k for k in t.kernels), t.kernels
    y.backward(tok(dy, O).to(dtype).cuda())
    torch.cuda.synchronize()
    _close(y, tok(ref, O), dtype)
    _close(xd.grad, tok(xr.grad, I), dtype)
    _close(wd.grad, wr.grad, dtype, fac=2)
    live = set(hip.conv3x3_dil_live_taps(H, W, d))
    gw = wd.grad.cpu()
    for tap in range(9):
        if tap not in live:
            assert (gw[:, :, tap // 3, tap % 3] == 0).all(), f'dead tap {tap} has a non-zero weight gradient'
            assert (wr.grad[:, :, tap // 3, tap % 3] == 0).all()
    if live == {4}:          # centre tap alone: the convolution IS the 1x1 product with the centre weights
        lin = Fh.linear(xd.detach(), wd.detach()[:, :, 1, 1].contiguous())
        _close(y, lin, dtype)
        _close(lin, tok(ref, O), dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('d', [12, 36])
def test_tap_culling_is_only_an_optimisation(d, dtype):
    """All three modes with SEGFAC_DILCONV_NO_CULL (nine taps, zero loads for the dead ones) and without agree within the fp32 bar."""
    from segmentation_factory_amd import hip
    B, H, W, I, O = 2, 16, 16, 256, 256
    P = B * H * W
    g = torch.Generator().manual_seed(70 + d)
    x = torch.randn(P, I, generator=g).to(dtype).cuda()
    dy = torch.randn(P, O, generator=g).to(dtype).cuda()
    wm = (torch.randn(O, 9 * I, generator=g) * (2.0 / (9 * I)) ** 0.5).to(dtype).cuda()
    wt = (torch.randn(I, 9 * O, generator=g) * (2.0 / (9 * O)) ** 0.5).to(dtype).cuda()

    def run():
        with hip.trace() as t:
            outs = (hip.conv3x3_dil(0, x, wm, B, H, W, I, O, d), hip.conv3x3_dil(1, dy, wt, B, H, W, I, O, d),
                    hip.conv3x3_dil(2, x, dy, B, H, W, I, O, d))
        torch.cuda.synchronize()
        assert sum('conv3x3_dil_kernel' in k for k in t.kernels) == 2 and any('conv3x3_dil_wgrad_kernel' in k for k in t.kernels), t.kernels
        return outs
    culled = run()
    with hip.policy_override(dilconv_no_cull=1):
        assert hip.policy('SEGFAC_DILCONV_NO_CULL') == 1
        full = run()
    for a, b in zip(culled, full):
        _close(a, b, torch.float32)
    dead = [t for t in range(9) if t not in hip.conv3x3_dil_live_taps(H, W, d)]
    assert len(dead) == (0 if d == 12 else 8)
    for dw in (culled[2], full[2]):
        for t in dead:
            assert (dw.view(O, 9, I)[:, t] == 0).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_elementwise_dropout(dtype):
    from segmentation_factory_amd import functional as Fh
    rows, cols, keep = 256, 256, 0.5                      # 2^16 elements
    g = torch.Generator().manual_seed(80)
    x = torch.randn(rows, cols, generator=g).to(dtype)
    dy = torch.randn(rows, cols, generator=g).to(dtype)
    owner = torch.nn.Dropout(1.0 - keep)
    xd = x.cuda().requires_grad_(True)
    assert Fh.dropout(xd, owner.p, False, owner) is xd                                   # eval: the identity
    mask = (torch.rand(rows, cols, generator=g) < keep).float()
    y = Fh.dropout(xd, owner.p, True, owner, override=mask)
    y.backward(dy.cuda())
    _close(y, x.float() * mask / keep, dtype)
    _close(xd.grad, dy.float() * mask / keep, dtype)
    assert ((y.float().cpu() == 0) | (mask == 1)).all()
    ones = torch.ones(rows, cols, dtype=dtype, device='cuda')
    a = Fh.dropout(ones, owner.p, True, owner).float().cpu()
    b = Fh.dropout(ones, owner.p, True, owner).float().cpu()
    assert set(a.unique().tolist()) <= {0.0, 1.0 / keep}
    sigma = (keep * (1 - keep) / (rows * cols)) ** 0.5                                    # 2^-9 for keep 0.5
    for t in (a, b):
        frac = (t != 0).float().mean().item()
        print(f'  kept fraction {frac:.5f} (keep {keep}, sigma {sigma:.5f})')
        assert abs(frac - keep) <= 4 * sigma
    assert not torch.equal(a, b)                                                          # consecutive draws differ


# ---- the head against the reference's recorded values ----------------------------------------------------------------------------------
FIXTURE = 'e2e_deeplabv3_mitb0_416x448.npz'
# Fraction `rt` of a parameter's gradient scale (the formula of tests/test_model_gpu.py::test_e2e_against_reference_golden).  The rule is
# "about twice the worst sample error / scale measured on the MI355X against the fixture", as GRAD_RT was set.  NOT MEASURED YET: these
# are the constants that rule gave the fixture of the same kind (batch 4, a BatchNorm head over a well-conditioned map, GRAD_RT
# 'convnext_128': measured 2e-3 / 0.133); the MiT-B0 backbone alone measured 1e-4 / 0.064.  The test prints the worst figure on every
# run: set these to twice that figure at the first GPU run and write it here and in DESIGN.md section 12.
DEEPLAB_GRAD_RT = {torch.float32: 5e-3, torch.bfloat16: 0.25}


def _zero_stochastic(model):
    for mod in model.modules():
        if hasattr(mod, 'drop_prob'):
            mod.drop_prob = 0.0
        if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)):
            mod.p = 0.0
    return model


def _fixture_model(golden_dir, dtype):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_deeplab_goldens import full_state_dict, load_inventory
    g = np.load(os.path.join(golden_dir, FIXTURE))
    nc = int(g['nc'])
    sd = full_state_dict(load_inventory(g), nc, int(g['seed']), int(g['head_seed']), str(g['backbone']))
    norms = [sd[str(k)].double().norm().item() for k in g['head_keys']]
    assert np.allclose(norms, g['head_weight_norms'], rtol=1e-12, atol=0), 'the head weights are not the ones the fixture was made with'
    m = SegmentationModel(str(g['backbone']), num_classes=nc, seg_head=str(g['head']), compute_dtype=dtype)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return g, _zero_stochastic(m.cuda())


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_deeplabv3_head_against_reference_golden(golden_dir, dtype):
    """MiT-B0 + DeepLabV3, batch 4 at 416 x 448 (13 x 14 top map), against the reference's captured values: head output in eval and
    train mode, a strided sample of the full-size eval logits, loss, sampled parameter gradients and gradient norms, BatchNorm step
    counters.  bf16: head.aspp.b4.* (a BatchNorm over the 4 samples of a 1 x 1 map) is held to gradient norms only."""
    from oracle import weights as OW
    from segmentation_factory_amd import criterion_lowres
    from tools.make_deeplab_goldens import sample_indices
    g, model = _fixture_model(golden_dir, dtype)
    nc, B, H, W, seed = int(g['nc']), int(g['B']), int(g['H']), int(g['W']), int(g['seed'])
    x, y = OW.synthetic_batch(B, H, W, nc, seed)
    fp32 = dtype == torch.float32
    rel = 1e-3 if fp32 else 5e-2
    model.eval()
    with torch.no_grad():
        ev = model(x.cuda()).cpu().numpy()
        lo = model.forward_lowres(x.cuda()).nchw().float().cpu().numpy()
    assert lo.shape == g['lowres_eval'].shape == (B, nc, 13, 14)
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
    rt = DEEPLAB_GRAD_RT[dtype]
    bad, worst, worst_norm = [], (0.0, ''), (0.0, '')
    for i, name in enumerate(g['grad_names']):
        name = str(name)
        gr = params[name].grad
        ref_norm = float(g['grad_norms'][i])
        assert gr is not None, name
        gr = gr.detach().float().cpu()
        got = gr.flatten()[sample_indices(name, gr.numel())].numpy()
        norm = gr.double().norm().item()
        if not fp32 and '.aspp.b4.' in name:
            if abs(norm - ref_norm) > 0.6 * ref_norm + 1e-1 * gmax:
                bad.append((name, norm, ref_norm))
            continue
        scale = np.abs(g['grad_samples'][i]).max() + ref_norm / max(1.0, np.sqrt(gr.numel())) + 1e-2 * gmax
        err = float(np.abs(got - g['grad_samples'][i]).max())
        nerr = abs(norm - ref_norm) / (ref_norm + 1e-1 * gmax)
        worst = max(worst, (err / scale, name))
        worst_norm = max(worst_norm, (nerr, name))
        if rt is not None and (err > rt * scale or nerr > rt):
            bad.append((name, err, rt * scale, norm, ref_norm))
    print(f'  worst gradient sample err/scale {worst[0]:.3e} ({worst[1]}); worst norm err {worst_norm[0]:.3e} ({worst_norm[1]})')
    assert rt is not None, 'DEEPLAB_GRAD_RT is not set'
    assert not bad, bad[:8]
    if fp32:
        sdn = model.state_dict()
        for i, name in enumerate(g['bn_names']):
            if str(name).endswith('num_batches_tracked'):       # two train-mode forwards ran above
                assert float(sdn[str(name)]) == 2 * float(g['bn_norms'][i]), str(name)


def test_deeplabv3_bn_running_stats_after_one_forward(golden_dir):
    """running_mean / running_var / num_batches_tracked after ONE train-mode forward vs the reference's buffers (fp32)."""
    from oracle import weights as OW
    g, model = _fixture_model(golden_dir, torch.float32)
    x, _ = OW.synthetic_batch(int(g['B']), int(g['H']), int(g['W']), int(g['nc']), int(g['seed']))
    model.train()
    model.forward_lowres(x.cuda())
    sdn = model.state_dict()
    n = 0
    for i, name in enumerate(g['bn_names']):
        v = sdn[str(name)]
        got = v.float().double().norm().item() if v.ndim else float(v)
        assert abs(got - float(g['bn_norms'][i])) <= 1e-4 * max(1.0, abs(float(g['bn_norms'][i]))), str(name)
        n += str(name).startswith('decode_head.')
    assert n == 3 * 7                                        # seven BatchNorms in the head


def test_deeplabv3_graphed_step(golden_dir, capsys):
    """Three steps of engine.train_one_epoch's default step (the captured hipGraph) with MiT-B0 + deeplabv3, batch 4, 64 x 64, 7 classes:
    finite losses, parameters move, and -- dropout rates 0, fp32 -- the first step's loss is the eager step's loss."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, criterion_lowres, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from tools.make_deeplab_goldens import full_state_dict, load_inventory
    g = np.load(os.path.join(golden_dir, FIXTURE))
    nc, B, H, W, seed = 7, 4, 64, 64, 9
    sd = full_state_dict(load_inventory(g), nc, seed, 77)
    x, y = OW.learnable_batch(B, H, W, nc, seed)
    args = types.SimpleNamespace(nb_classes=nc, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)

    def build(zero):
        m = SegmentationModel('MiT-B0', num_classes=nc, seg_head='deeplabv3', compute_dtype=torch.float32)
        m.load_state_dict(sd, strict=True)
        m = m.cuda()
        return _zero_stochastic(m) if zero else m

    def run(model, steps=3):
        opt = FusedAGCAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        losses = []

        class Rec:
            def add_scalar(self, name, v, it=None):
                if name == 'train_loss':
                    losses.append(float(v))
        engine.train_one_epoch(model, opt, [(x, y)] * steps, 0, 'cuda', 1, None, None, NativeScaler(), Rec(), args)
        return losses

    eager = build(True).train()
    l_eager = criterion_lowres(eager.forward_lowres(x.cuda()), y.cuda(), (H, W), None, num_classes=nc, dice=True, ignore_index=255).item()
    model = build(True)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    losses = run(model)
    assert getattr(model, '_graphed_step', None) is not None and 'captured as one hipGraph' in capsys.readouterr().out
    print(f'  graphed losses {losses}, eager first loss {l_eager:.7f}')
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert abs(losses[0] - l_eager) <= 1e-5 * max(1.0, abs(l_eager))
    moved = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:8]
    # with the dropouts live the graph still captures and replays (fresh masks from the device-side generator)
    live = build(False)
    l_live = run(live)
    assert getattr(live, '_graphed_step', None) is not None and len(l_live) == 3 and all(np.isfinite(l_live))
