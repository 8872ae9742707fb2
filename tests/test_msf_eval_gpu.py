"""Multi-scale + flip evaluation on the GPU: segf_msf_argmax_confmat (csrc/eval_msf.hip) against the float64 torch restatement of
tests/msf_refs.py, and engine.evaluate_msf / Metrics.update_msf / SemSeg.predict on top of it.

Probabilities: prob_out against oracle(float64) within max(8 e32, 4e-6), e32 = the error of oracle(float32) against oracle(float64)
on the same inputs (torch alone sets the yardstick; the e32 values seen on the MI355X are recorded in profiles/msf_eval.md).
Predictions: equal to the float64 arg max outside the tie band (float64 top-2 margin below 1e-4; at most 0.5 % of the pixels);
counts: equal to a bincount of (target, pred_out) on ALL pixels, which checks the counting independently of ties."""
import types

import pytest
import torch
import torch.nn.functional as F

import msf_refs as R

pytestmark = pytest.mark.gpu

STORAGE = [torch.float32, torch.bfloat16]
H, W = R.STANDARD_HW
B = R.STANDARD_B


def _check_against_oracle(maps, flips, C, Hh, Ww, label, **kw):
    """prob_out within the derived tolerance of the float64 oracle, pred_out equal to its arg max outside the tie band."""
    S64 = R.oracle(maps, flips, Hh, Ww, torch.float64)
    e32 = (R.oracle(maps, flips, Hh, Ww, torch.float32).double() - S64).abs().max().item()
    out = R.run_kernel(maps, flips, C, Hh, Ww, **kw)
    err = (out['prob'].double() - S64.permute(0, 2, 3, 1)).abs().max().item()
    band = R.tie_band(S64)
    wrong = ((out['pred'] != S64.argmax(1)) & ~band).sum().item()
    print(f'[msf {label}] e32 {e32:.3e} atol {R.prob_atol(e32):.3e} kernel err {err:.3e} tie band {band.float().mean().item():.4%} '
          f'wrong outside the band {wrong}')
    assert err <= R.prob_atol(e32), (label, err, e32)
    assert band.float().mean().item() <= R.TIE_SHARE
    assert wrong == 0
    return out, S64


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C,amp', [(2, 3.0), (19, 3.0), (64, 3.0), (150, 3.0), (192, 3.0), (150, 8.0)])
def test_probabilities_against_float64(C, amp, storage):
    maps, flips, S64, e32 = R.standard_case(C, amp, storage)
    out = R.run_kernel(maps, flips, C, H, W)
    err = (out['prob'].double() - S64.permute(0, 2, 3, 1)).abs().max().item()
    print(f'[msf prob C={C} amp={amp} {storage}] e32 {e32:.3e} atol {R.prob_atol(e32):.3e} kernel err {err:.3e}')
    assert err <= R.prob_atol(e32), (err, e32)
    total = out['prob'].sum(-1)                                    # every pixel's sums add up to the number of maps
    assert (total - len(maps)).abs().max().item() <= 1e-4


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C,ignore_label,bad_label', [(19, 255, None), (150, 255, None), (19, 3, None), (19, 255, 200), (2, 255, None)],
                         ids=['C19', 'C150', 'ignore-in-range', 'bad-label', 'C2'])
def test_predictions_and_counts(C, ignore_label, bad_label, storage):
    maps, flips, S64, _ = R.standard_case(C, 3.0, storage)
    target = R.make_target(B, H, W, C, ignore_label, bad_label)
    out = R.run_kernel(maps, flips, C, H, W, target=target, ignore_label=ignore_label)
    band = R.tie_band(S64)
    share = band.float().mean().item()
    print(f'[msf pred C={C} {storage}] tie band {share:.4%}')
    assert share <= R.TIE_SHARE
    assert torch.equal(out['pred'][~band], S64.argmax(1)[~band])
    mat, hist = R.counts(target, out['pred'], C, ignore_label)
    assert torch.equal(out['mat'], mat) and torch.equal(out['hist'], hist)
    in_range = ((target >= 0) & (target < C))
    assert out['mat'].sum().item() == in_range.sum().item()
    assert out['hist'].sum().item() == (in_range & (target != ignore_label)).sum().item()
    assert out['flag'] == (1 if bad_label is not None else 0)       # the bad label is flagged and (sums above) counted nowhere
    if 0 <= ignore_label < C:
        assert out['mat'][ignore_label].sum() > 0 and out['hist'][ignore_label].sum() == 0


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('geom', [(5, 7), (12, 20)], ids=['5x7', '12x20'])
def test_flip_is_exact(geom, storage):
    """A map with flip = 1 and its mirrored copy with flip = 0 are the same sample: bit-identical sums."""
    C = 19
    m, = R.make_maps(B, C, [geom + (0,)], 3.0, storage, seed=3)
    a = R.run_kernel([m], [1], C, H, W)
    b = R.run_kernel([m.flip(2).contiguous()], [0], C, H, W)
    assert torch.equal(a['prob'], b['prob']) and torch.equal(a['pred'], b['pred'])
    c = R.run_kernel([m], [0], C, H, W)
    assert not torch.equal(a['prob'], c['prob'])                    # and the flag does something


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
def test_one_map_reduces_to_argmax_confmat(storage):
    """n = 1, no flip, ratio 4: softmax is monotonic, so the counts are segf_argmax_confmat's.  Noise of amplitude 0.1 plus 5 on one
    class per low-resolution pixel: the winner's margin is at least 5 (5/8 - 3/8) - 0.2 = 1.05 everywhere, no tie can differ."""
    from segmentation_factory_amd import hip
    C, h, w = 19, 6, 10
    g = torch.Generator().manual_seed(5)
    m = 0.1 * (2 * torch.rand(B, h, w, C, generator=g) - 1)
    win = torch.randint(0, C, (B, h, w), generator=g)
    m.scatter_add_(3, win.unsqueeze(-1), torch.full((B, h, w, 1), 5.0))
    m = m.to(storage)
    target = R.make_target(B, H, W, C)
    out = R.run_kernel([m], [0], C, H, W, target=target)
    mat = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.empty((B, H, W), dtype=torch.int64, device='cuda')
    hip.argmax_confmat(m.reshape(B * h * w, C).cuda(), B, C, h, w, H, W, target.cuda(), 255, mat, hist, flag, pred)
    assert torch.equal(out['mat'], mat.cpu()) and torch.equal(out['hist'], hist.cpu())
    assert torch.equal(out['pred'], pred.cpu())
    assert out['mat'].sum() > 0


def test_determinism_and_order():
    C = 150
    maps, flips, S64, e32 = R.standard_case(C, 3.0, torch.bfloat16)
    a = R.run_kernel(maps, flips, C, H, W)
    b = R.run_kernel(maps, flips, C, H, W)
    assert torch.equal(a['prob'], b['prob']) and torch.equal(a['pred'], b['pred'])
    perm = [4, 0, 6, 2, 5, 1, 3]
    c = R.run_kernel([maps[i] for i in perm], [flips[i] for i in perm], C, H, W)
    d = (c['prob'] - a['prob']).abs().max().item()
    print(f'[msf order] permuting the maps moves prob_out by {d:.3e} (atol {R.prob_atol(e32):.3e})')
    assert d <= R.prob_atol(e32)


@pytest.mark.parametrize('case', ['1x1', 'W3-w2-flip', 'n16', 'C65', 'ldl=C+3'])
def test_shapes_that_can_go_wrong(case):
    if case == '1x1':
        maps = R.make_maps(1, 19, [(1, 1, 0)], 3.0, torch.float32, seed=7)
        _check_against_oracle(maps, [0], 19, 1, 1, case)
    elif case == 'W3-w2-flip':
        maps = R.make_maps(2, 19, [(2, 2, 1), (3, 2, 0)], 3.0, torch.bfloat16, seed=8)
        _check_against_oracle(maps, [1, 0], 19, 5, 3, case)
    elif case == 'n16':
        geoms = [(3 + k, 4 + 2 * k, k & 1) for k in range(16)]
        maps = R.make_maps(2, 19, geoms, 3.0, torch.bfloat16, seed=9)
        out, _ = _check_against_oracle(maps, [f for _, _, f in geoms], 19, 12, 20, case)
        assert (out['prob'].sum(-1) - 16).abs().max().item() <= 1e-4
    elif case == 'C65':
        geoms = [(6, 10, 0), (5, 7, 1), (24, 40, 1)]
        maps = R.make_maps(2, 65, geoms, 3.0, torch.float32, seed=10)
        maps[0][..., 64] += 6.0                                      # the one class of the second slot wins often
        out, _ = _check_against_oracle(maps, [0, 1, 1], 65, 24, 40, case)
        assert (out['pred'] == 64).float().mean().item() > 0.05
    else:
        geoms = [(6, 10, 0), (5, 7, 1), (24, 40, 0)]
        maps = R.make_maps(2, 19, geoms, 3.0, torch.float32, seed=11)
        _check_against_oracle(maps, [0, 1, 0], 19, 24, 40, case, ldl=19 + 3)


def test_no_target_means_no_counting():
    from segmentation_factory_amd import hip
    C = 19
    maps, flips, S64, _ = R.standard_case(C, 3.0, torch.float32)
    rows = [(m.reshape(-1, C).cuda(), m.shape[1], m.shape[2]) for m in maps]
    mat = torch.full((C, C), 7, dtype=torch.int64, device='cuda')
    hist = torch.full((C, C), 9, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device='cuda')
    hip.msf_argmax_confmat(rows, flips, B, C, H, W, None, 255, mat, hist, flag, pred_out=pred)
    band = R.tie_band(S64)
    assert torch.equal(pred.cpu()[~band], S64.argmax(1)[~band]) and int(pred.min()) >= 0
    assert bool((mat == 7).all()) and bool((hist == 9).all()) and int(flag.item()) == 0


# ---- end to end: MiT-B0 + SegFormerHead, B = 2, 64 x 96, scales (0.5, 1.0, 1.5) + flip -------------------------------------------
NC, SCALES = 7, (0.5, 1.0, 1.5)


@pytest.fixture(scope='module')
def e2e():
    """Model, batch and the manual loop's result (one forward_lowres per scale and flip, one update_msf), computed once."""
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, engine, hip, utils
    from segmentation_factory_amd.metrics import Metrics
    model = SegmentationModel('MiT-B0', num_classes=NC, seg_head='SegFormerHead', compute_dtype=torch.float32)
    model.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', NC, 77, lively=True))
    model = model.cuda().eval()
    x, y = OW.synthetic_batch(2, 64, 96, NC, 78)                     # labels with an ignored band and ~2 % ignored pixels
    x, y = x.cuda(), y.cuda()
    maps, flips = [], []
    with torch.inference_mode():
        for size in engine.msf_sizes(64, 96, SCALES):
            xs = x if size == (64, 96) else F.interpolate(x, size=size, mode='bilinear', align_corners=False)
            for f in (0, 1):
                lo = model.forward_lowres(xs.flip(3) if f else xs)
                maps.append(types.SimpleNamespace(data=lo.data.clone(), B=lo.B, H=lo.H, W=lo.W))
                flips.append(f)
        metric, confmat = Metrics(NC, 255, 'cuda'), utils.ConfusionMatrix(NC)
        metric.update_msf(maps, flips, y, (64, 96), confmat=confmat)
        pred = torch.empty((2, 64, 96), dtype=torch.int64, device='cuda')
        z = torch.zeros((NC, NC), dtype=torch.int64, device='cuda')
        hip.msf_argmax_confmat(maps, flips, 2, NC, 64, 96, y, 255, z, z.clone(), torch.zeros(1, dtype=torch.int32, device='cuda'),
                               pred_out=pred)
        # the aliasing trap is visible on this input: were the straight result overwritten by the mirrored one, the counts would differ
        aliased, c2 = Metrics(NC, 255, 'cuda'), utils.ConfusionMatrix(NC)
        aliased.update_msf([maps[k | 1] for k in range(len(maps))], flips, y, (64, 96), confmat=c2)
    assert [(m.H, m.W) for m in maps[::2]] == [(8, 16), (16, 24), (24, 40)]
    assert not torch.equal(aliased.hist, metric.hist)
    return types.SimpleNamespace(model=model, x=x, y=y, maps=maps, flips=flips, hist=metric.hist.cpu().clone(),
                                 mat=confmat.mat.cpu().clone(), pred=pred.cpu())


def _args(**kw):
    return types.SimpleNamespace(nb_classes=NC, ignore_label=255, **kw)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_evaluate_msf_matches_the_manual_loop(e2e, graph):
    """The loader yields the same batch twice.  With the graph on, the first batch runs each scale eagerly (straight) and captures it
    (mirrored), the second replays both from ONE static output buffer per scale: the aliasing trap.  Both sightings must add the manual
    loop's counts."""
    from segmentation_factory_amd import engine
    confmat, metric = engine.evaluate_msf(_args(hip_graph=graph), e2e.model, [(e2e.x, e2e.y)] * 2, 'cuda', 10, None, scales=SCALES, flip=True)
    assert e2e.hist.sum() > 0
    assert torch.equal(metric.hist.cpu(), 2 * e2e.hist)
    assert torch.equal(confmat.mat.cpu(), 2 * e2e.mat)
    if graph:
        # every scale now has its graph: a further sighting (all replays) adds the same increment again
        assert len(e2e.model.__dict__['_graphed_eval']['graphs']) == len(SCALES)
        confmat1, metric1 = engine.evaluate_msf(_args(hip_graph=True), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10, None, scales=SCALES, flip=True)
        assert torch.equal(metric1.hist.cpu(), e2e.hist) and torch.equal(confmat1.mat.cpu(), e2e.mat)


def test_evaluate_dispatches_on_the_flags_only(e2e):
    from segmentation_factory_amd import engine, utils
    from segmentation_factory_amd.metrics import Metrics
    confmat, metric = engine.evaluate(_args(hip_graph=False, eval_scales=list(SCALES), eval_flip=True), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert torch.equal(metric.hist.cpu(), e2e.hist) and torch.equal(confmat.mat.cpu(), e2e.mat)
    # no flags (absent, or the CLI's defaults): the single-forward path, i.e. a direct update_lowres loop
    m0, c0 = Metrics(NC, 255, 'cuda'), utils.ConfusionMatrix(NC)
    with torch.inference_mode():
        m0.update_lowres(e2e.model.forward_lowres(e2e.x), e2e.y, (64, 96), confmat=c0)
    for a in (_args(hip_graph=False), _args(hip_graph=False, eval_scales=None, eval_flip=False)):
        confmat, metric = engine.evaluate(a, e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
        assert torch.equal(metric.hist.cpu(), m0.hist.cpu()) and torch.equal(confmat.mat.cpu(), c0.mat.cpu())
    assert not torch.equal(m0.hist.cpu(), e2e.hist)                  # MSF is a different prediction


def test_e2e_predictions_against_float64(e2e):
    maps = [m.data.view(m.B, m.H, m.W, NC).cpu() for m in e2e.maps]
    S64 = R.oracle(maps, e2e.flips, 64, 96, torch.float64)
    band = R.tie_band(S64)
    print(f'[msf e2e] tie band {band.float().mean().item():.4%}')
    assert band.float().mean().item() <= R.TIE_SHARE
    assert torch.equal(e2e.pred[~band], S64.argmax(1)[~band])


def test_semseg_predict_msf(e2e):
    """SemSeg.predict(scales=..., flip=True): the kernel's pred_out for that image (maps resampled to the ORIGINAL size)."""
    from segmentation_factory_amd import engine
    from segmentation_factory_amd.inference import SemSeg
    ss = SemSeg(e2e.model, img_size=64)
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (3, 50, 70), generator=g, dtype=torch.uint8)
    seg, col = ss.predict(img, overlay=False, scales=(0.5, 1.0), flip=True)
    assert seg.shape == (50, 70) and seg.dtype == torch.int64 and col is None
    x = ss.preprocess(img)
    maps, flips = [], []
    with torch.inference_mode():
        for size in engine.msf_sizes(x.shape[2], x.shape[3], (0.5, 1.0)):
            xs = x if size == tuple(x.shape[2:]) else F.interpolate(x, size=size, mode='bilinear', align_corners=False)
            for f in (0, 1):
                lo = e2e.model.forward_lowres(xs.flip(3) if f else xs)
                maps.append(lo.data.view(1, lo.H, lo.W, NC).cpu())
                flips.append(f)
    S64 = R.oracle(maps, flips, 50, 70, torch.float64)
    band = R.tie_band(S64)
    assert band.float().mean().item() <= R.TIE_SHARE
    assert torch.equal(seg.cpu()[~band[0]], S64.argmax(1)[0][~band[0]])
    plain, _ = ss.predict(img, overlay=False)
    assert plain.shape == seg.shape
