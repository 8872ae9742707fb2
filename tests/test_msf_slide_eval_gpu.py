"""Multi-scale + flip sliding-window evaluation on the GPU: segf_msf_slide_argmax_confmat (csrc/eval_msf_slide.hip) against the
float64 torch restatement of tests/msf_slide_refs.py, and engine.evaluate_msf_slide / Metrics.update_msf_slide /
SemSeg.predict(msf_slide=...) on top of it.

Summed probabilities: prob_out against oracle(float64) within msf_refs.prob_atol(e32) = max(8 e32, 4e-6), e32 = the error of the
float32 restatement (the same two resamplings, the same division, the same softmax in fp32) against the float64 one on the same
inputs.  Predictions: equal to the float64 arg max wherever the float64 top-2 margin of the sum is at least TIE_MARGIN; the pixels
inside that band are at most 0.5 % (asserted on the reference alone, first).  Counts: equal to a bincount of (target, pred_out) on ALL
pixels, which checks the counting independently of ties.  The figures seen on the MI355X are recorded in
profiles/msf_slide_eval.md."""
import types

import pytest
import torch
import torch.nn.functional as F

import msf_refs
import msf_slide_refs as R
import slide_refs

pytestmark = pytest.mark.gpu

STORAGE = [torch.float32, torch.bfloat16]
B = R.STANDARD_B
H, W = R.STANDARD_HW


def _check(tag, S64, e32, out):
    """The numerical bar of one kernel result against a reference; the figures are printed before the assertions."""
    band = R.tie_band(S64)
    share = band.float().mean().item()
    err = (out['prob'].double() - S64.permute(0, 2, 3, 1)).abs().max().item()
    wrong = ((out['pred'] != S64.argmax(1)) & ~band).sum().item()
    print(f'[msf-slide {tag}] e32 {e32:.3e} atol {R.prob_atol(e32):.3e} kernel err {err:.3e} tie band {share:.4%} '
          f'wrong outside the band {wrong}')
    assert share <= R.TIE_SHARE                      # a condition on the reference alone
    assert err <= R.prob_atol(e32), (tag, err, R.prob_atol(e32))
    assert wrong == 0


@pytest.mark.parametrize('amp', [3.0, 8.0], ids=['amp3', 'amp8'])
@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [7, 19, 64, 100, 150])
def test_standard_case_against_float64(C, storage, amp):
    sets, S64, e32 = R.standard_case(C, amp, storage)
    out = R.run_kernel(sets, C, H, W)
    _check(f'C{C} {storage} amp {amp}', S64, e32, out)


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [7, 19, 150])
def test_counts(C, storage):
    """mat / hist / flag against a bincount of (target, pred_out) on every pixel: ignored and bad labels, padded rows with poison in
    the pad columns (ldl > C, ldp > C), the counting-only call, and no target = no counting."""
    sets, S64, e32 = R.standard_case(C, 3.0, storage)
    plain = R.run_kernel(sets, C, H, W)
    for bad in (None, 200, -3):
        tg = R.make_target(B, H, W, C, 255, bad_label=bad)
        full = R.run_kernel(sets, C, H, W, target=tg, ldl=C + 5, ldp=C + 3)
        assert torch.equal(full['pred'], plain['pred']) and torch.equal(full['prob'], plain['prob'])     # the pad columns are never read
        mat, hist = R.counts(tg, full['pred'], C, 255)
        assert torch.equal(full['mat'], mat) and torch.equal(full['hist'], hist)
        assert full['flag'] == (0 if bad is None else 1)
        assert int(mat.sum()) == int(((tg >= 0) & (tg < C)).sum()) and int(hist.sum()) > 0
        only = R.run_kernel(sets, C, H, W, target=tg, want_pred=False, want_prob=False)
        assert torch.equal(only['mat'], mat) and torch.equal(only['hist'], hist) and only['flag'] == full['flag']
    assert int(plain['mat'].sum()) == 0 and int(plain['hist'].sum()) == 0 and plain['flag'] == 0
    assert int(plain['pred'].min()) >= 0 and int(plain['pred'].max()) < C


def test_label_equal_to_a_class_that_is_ignored():
    """ignore_label inside [0, C): counted in mat, not in hist (eval_count)."""
    C = 19
    sets, _, _ = R.standard_case(C, 3.0, torch.float32)
    tg = R.make_target(B, H, W, C, ignore_label=4)
    out = R.run_kernel(sets, C, H, W, target=tg, ignore_label=4)
    mat, hist = R.counts(tg, out['pred'], C, 4)
    assert torch.equal(out['mat'], mat) and torch.equal(out['hist'], hist) and out['flag'] == 0
    assert int(hist[4].sum()) == 0 and int(mat[4].sum()) > 0


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [19, 150])
def test_one_window_per_set_is_the_msf_kernel(C, storage):
    """Sets 1 and 4 of the standard case, each with a crop >= its image: one window, so the window mean is the window's sample and
    the call is msf_argmax_confmat's on the same maps -- predictions and counts outside the tie band, prob_out within prob_atol."""
    geoms = [((24, 40), (24, 40), (24, 40), (4, 4), 1), ((24, 40), (32, 64), (11, 11), (6, 10), 0)]
    sets = R.make_sets(B, C, geoms, storage, 3.0, seed0=11)
    assert all(s['maps'].shape[1] == 1 and s['crop'] == (24, 40) for s in sets)
    S64, e32 = R.reference(sets, H, W)
    band = R.tie_band(S64)
    tg = R.make_target(B, H, W, C, 255, bad_label=200)
    tg[band] = 255                                                     # the band is counted nowhere: the counts must then agree exactly
    out = R.run_kernel(sets, C, H, W, target=tg)
    _check(f'one-window C{C} {storage}', S64, e32, out)
    msf = msf_refs.run_kernel([s['maps'][:, 0] for s in sets], [s['flip'] for s in sets], C, H, W, target=tg)
    diff = (out['prob'] - msf['prob']).abs().max().item()
    print(f'[msf-slide one-window C{C} {storage}] against msf_argmax_confmat: max diff {diff:.3e}, bit-identical '
          f'{torch.equal(out["prob"], msf["prob"])}')
    assert diff <= R.prob_atol(e32)
    assert torch.equal(out['pred'][~band], msf['pred'][~band])
    assert torch.equal(out['mat'], msf['mat']) and torch.equal(out['hist'], msf['hist']) and out['flag'] == msf['flag'] == 1


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [19, 150])
def test_one_straight_same_size_set_is_the_slide_kernel(C, storage):
    """One un-flagged set at the output size: prob_out is the softmax of slide_argmax_confmat's mean_out.  (The seed is one at which
    the reference-only tie-band condition holds for both storages: a single softmax over 150 classes has small top-2 margins, and at
    seeds 11 and 12 the float64 band holds 0.52 % of the pixels.)"""
    sets = R.make_sets(B, C, [((24, 40), (16, 16), (11, 11), (4, 4), 0)], storage, 3.0, seed0=14)
    S64, e32 = R.reference(sets, H, W)
    out = R.run_kernel(sets, C, H, W)
    _check(f'one-set C{C} {storage}', S64, e32, out)
    sl = slide_refs.run_kernel(sets[0]['maps'], C, H, W, sets[0]['crop'], sets[0]['stride'])
    want = sl['mean'].softmax(3)
    diff = (out['prob'] - want).abs().max().item()
    print(f'[msf-slide one-set C{C} {storage}] against softmax(slide mean_out): max diff {diff:.3e}')
    assert diff <= R.prob_atol(e32)
    band = R.tie_band(S64)
    assert torch.equal(out['pred'][~band], sl['pred'][~band])


@pytest.mark.parametrize('out_hw', [(16, 40), (24, 56), (9, 23)], ids=['same-size', 'up', 'down'])
@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
def test_flip_is_exact(storage, out_hw):
    """ny = 1, origins 0, 12, 24 over 40 columns (a symmetric grid), direct inner read: the mirrored windows in mirrored order with
    the flag give the bits of the plain windows without it -- every pixel is covered at most twice and a + b = b + a."""
    C, size, crop, stride = 19, (16, 40), (16, 16), (12, 12)
    ny, nx, origins = slide_refs.windows_of(16, 40, crop, stride)
    assert (ny, nx) == (1, 3) and [x for _, x in origins] == [0, 12, 24]
    maps = slide_refs.make_maps(B, C, 3, 16, 16, storage, seed=5, amp=3.0)
    mirrored = maps.flip(1).flip(3).contiguous()                      # window order reversed, every window mirrored (axis 3 = columns)
    plain = R.run_kernel([dict(maps=maps, size=size, crop=crop, stride=stride, flip=0)], C, *out_hw)
    flagged = R.run_kernel([dict(maps=mirrored, size=size, crop=crop, stride=stride, flip=1)], C, *out_hw)
    assert torch.equal(plain['prob'], flagged['prob']) and torch.equal(plain['pred'], flagged['pred'])
    unflagged = R.run_kernel([dict(maps=mirrored, size=size, crop=crop, stride=stride, flip=0)], C, *out_hw)
    assert not torch.equal(plain['prob'], unflagged['prob'])           # the flag is what undoes the mirroring
    if out_hw == size:                                                  # no outer weights: without the flag the result is the mirrored map
        assert torch.equal(plain['prob'], unflagged['prob'].flip(2))


def test_determinism_and_no_allocation():
    from segmentation_factory_amd import hip
    C = 150
    sets, _, _ = R.standard_case(C, 3.0, torch.bfloat16)
    wsets = [(R.device_rows(s['maps'], C), s['size'], s['crop'], s['stride']) for s in sets]
    flips = [s['flip'] for s in sets]
    tg = R.make_target(B, H, W, C, 255).cuda()
    bufs = []
    for _ in range(2):
        bufs.append(dict(mat=torch.zeros((C, C), dtype=torch.int64, device='cuda'), hist=torch.zeros((C, C), dtype=torch.int64, device='cuda'),
                         flag=torch.zeros(1, dtype=torch.int32, device='cuda'), pred=torch.empty((B, H, W), dtype=torch.int64, device='cuda'),
                         prob=torch.empty((B * H * W, C), dtype=torch.float32, device='cuda')))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for b in bufs:
        hip.msf_slide_argmax_confmat(wsets, flips, B, C, H, W, tg, 255, b['mat'], b['hist'], b['flag'], pred_out=b['pred'], prob_out=b['prob'])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before
    assert torch.equal(bufs[0]['prob'], bufs[1]['prob']) and torch.equal(bufs[0]['pred'], bufs[1]['pred'])
    assert torch.equal(bufs[0]['mat'], bufs[1]['mat']) and torch.equal(bufs[0]['hist'], bufs[1]['hist'])
    assert int(bufs[0]['hist'].sum()) > 0


def test_layout_checks_of_the_binding():
    from segmentation_factory_amd import hip
    C = 19
    rows = torch.zeros((2 * 6 * 12, C), device='cuda')                # B 2, grid 2 x 3 over 20 x 29, maps 3 x 4
    pred = torch.empty((2, 24, 40), dtype=torch.int64, device='cuda')
    good = ((rows, 3, 4), (20, 29), (12, 16), (8, 9))
    call = lambda sets, flips=None: hip.msf_slide_argmax_confmat(sets, flips if flips is not None else [0] * len(sets), 2, C, 24, 40, None,
                                                                 255, None, None, None, pred_out=pred)
    call([good, good])
    with pytest.raises(ValueError):                                   # one flag short
        call([good, good], [0])
    with pytest.raises(ValueError):                                   # one window short
        call([good, ((rows[:-12], 3, 4),) + good[1:]])
    with pytest.raises(ValueError):                                   # fewer columns than classes
        call([((rows[:, :18], 3, 4),) + good[1:]])
    with pytest.raises(ValueError):                                   # inner stride 2
        call([((torch.zeros((144, 38), device='cuda')[:, ::2], 3, 4),) + good[1:]])
    with pytest.raises(ValueError):                                   # stride larger than the crop
        call([((rows, 3, 4), (20, 29), (12, 16), (13, 9))])
    with pytest.raises(ValueError):                                   # two dtypes
        call([good, ((rows.bfloat16(), 3, 4),) + good[1:]])
    with pytest.raises(ValueError):                                   # an unclamped crop
        call([((rows, 3, 4), (20, 29), (32, 16), (8, 9))])
    with pytest.raises(RuntimeError):                                 # 17 sets: refused by the library
        call([good] * 17)


# ---- end to end: MiT-B0 + SegFormerHead, B = 2, 96 x 160, crop 64, stride 48, scales 0.5 / 1.0 / 1.5, mirrored ---------------------
NC, HI, WI, CROP, STRIDE, SCALES = 7, 96, 160, 64, 48, (0.5, 1.0, 1.5)


def _manual_sets(model, x, scales, flip):
    """The manual loop: per scale and flip ONE forward_lowres per window (batch 1), rows stacked image-major, then window order.
    -> ([(rows, h, w), size, crop, stride], flips)"""
    from segmentation_factory_amd import engine
    nb = x.shape[0]
    sets, flips = [], []
    for size in engine.msf_sizes(x.shape[2], x.shape[3], scales):
        xs = x if size == tuple(x.shape[2:]) else F.interpolate(x, size=size, mode='bilinear', align_corners=False)
        (ch, cw), strd, origins = engine.slide_windows(size[0], size[1], CROP, STRIDE)
        for f in ((0, 1) if flip else (0,)):
            src = xs.flip(3) if f else xs
            rows = []
            for b in range(nb):
                for oy, ox in origins:
                    lo = model.forward_lowres(src[b:b + 1, :, oy:oy + ch, ox:ox + cw].contiguous())
                    rows.append(lo.data[:, :NC].clone())
            sets.append(((torch.cat(rows).contiguous(), lo.H, lo.W), size, (ch, cw), strd))
            flips.append(f)
    return sets, flips


@pytest.fixture(scope='module')
def e2e():
    """Model, batch and the manual loop's result (one forward_lowres per window, one update_msf_slide), computed once."""
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, engine, hip, utils
    from segmentation_factory_amd.metrics import Metrics
    model = SegmentationModel('MiT-B0', num_classes=NC, seg_head='SegFormerHead', compute_dtype=torch.float32)
    model.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', NC, 77, lively=True))
    model = model.cuda().eval()
    x, y = OW.synthetic_batch(2, HI, WI, NC, 78)                     # labels with an ignored band and ~2 % ignored pixels
    x, y = x.cuda(), y.cuda()
    assert engine.msf_sizes(HI, WI, SCALES) == [(64, 96), (96, 160), (160, 256)]
    with torch.inference_mode():
        sets, flips = _manual_sets(model, x, SCALES, True)
        assert flips == [0, 1, 0, 1, 0, 1]
        assert [s[0][0].shape[0] // (2 * 256) for s in sets] == [2, 2, 6, 6, 15, 15]        # windows per image; every window 64 x 64 -> 16 x 16

        def count(ss):
            metric, confmat = Metrics(NC, 255, 'cuda'), utils.ConfusionMatrix(NC)
            metric.update_msf_slide(ss, flips, y, (HI, WI), confmat=confmat)
            return metric.hist.cpu().clone(), confmat.mat.cpu().clone()
        hist, mat = count(sets)
        pred = torch.empty((2, HI, WI), dtype=torch.int64, device='cuda')
        hip.msf_slide_argmax_confmat(sets, flips, 2, NC, HI, WI, None, 255, None, None, None, pred_out=pred)
        # the aliasing traps are visible on this input.  All windows are 64 x 64, so under a graph every forward of a chunk shape
        # comes out of ONE static buffer:
        swap = lambda k, rows: ((rows, 16, 16),) + sets[k][1:]
        # (a) the mirrored result stands in for the straight one, at every scale
        mirrored_hist, _ = count([swap(k, sets[k | 1][0][0]) for k in range(6)])
        # (b) the windows of scale 1.5 stand in for those of scale 1.0 (same window shape, another image content)
        n10 = sets[2][0][0].shape[0]
        other_hist, _ = count([swap(k, sets[4][0][0][:n10].contiguous()) if k == 2 else sets[k] for k in range(6)])
        # (c) with window_batch = 4 the 12 straight windows of scale 1.0 travel as 3 chunks of 4: each one replay late
        chunks = sets[2][0][0].view(3, 4 * 256, NC)
        stale_hist, _ = count([swap(k, torch.cat([chunks[0], chunks[0], chunks[1]]).contiguous()) if k == 2 else sets[k] for k in range(6)])
    assert hist.sum() > 0
    assert not torch.equal(mirrored_hist, hist) and not torch.equal(other_hist, hist) and not torch.equal(stale_hist, hist)
    return types.SimpleNamespace(model=model, x=x, y=y, sets=sets, flips=flips, hist=hist, mat=mat, pred=pred.cpu())


def _args(**kw):
    return types.SimpleNamespace(nb_classes=NC, ignore_label=255, **kw)


@pytest.mark.parametrize('window_batch', [None, 4, 5], ids=['all', 'chunks-of-4', 'chunks-of-5'])
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_evaluate_msf_slide_matches_the_manual_loop(e2e, graph, window_batch):
    """The loader yields the same batch twice.  With the graph on, a chunk shape is captured on its second sighting -- inside the
    first batch already, since all scales and both flips share the window shape -- and replayed from then on out of ONE static output
    buffer.  Both batches must add the manual loop's counts, whatever the chunking."""
    from segmentation_factory_amd import engine
    confmat, metric = engine.evaluate_msf_slide(_args(hip_graph=graph), e2e.model, [(e2e.x, e2e.y)] * 2, 'cuda', 10, None, scales=SCALES,
                                                flip=True, crop=CROP, stride=STRIDE, window_batch=window_batch)
    assert torch.equal(metric.hist.cpu(), 2 * e2e.hist)
    assert torch.equal(confmat.mat.cpu(), 2 * e2e.mat)


def test_evaluate_dispatches_on_eval_mode(e2e):
    from segmentation_factory_amd import engine
    a = _args(hip_graph=False, eval_mode='slide-msf', eval_crop=[CROP], eval_stride=[STRIDE], eval_window_batch=4, eval_scales=list(SCALES),
              eval_flip=True)
    confmat, metric = engine.evaluate(a, e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert torch.equal(metric.hist.cpu(), e2e.hist) and torch.equal(confmat.mat.cpu(), e2e.mat)
    # without the flip: other counts, the same number of counted pixels
    a = _args(hip_graph=False, eval_mode='slide-msf', eval_crop=[CROP], eval_stride=[STRIDE], eval_scales=list(SCALES))
    confmat, metric = engine.evaluate(a, e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert metric.hist.sum() == e2e.hist.sum() and not torch.equal(metric.hist.cpu(), e2e.hist)


def test_one_scale_one_window_is_evaluate(e2e):
    """scales (1.0,), no flip, crop >= image: one window and one map, and the arg max of a softmax is the arg max of the logits
    except on rounding ties -- the counted pixels are evaluate's, and the matrices differ by no more pixels than the float64 tie band
    of this map holds."""
    from segmentation_factory_amd import engine
    c0, m0 = engine.evaluate(_args(hip_graph=False), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    with torch.inference_mode():
        lo = e2e.model.forward_lowres(e2e.x)
    maps = lo.data[:, :NC].cpu().view(2, 1, lo.H, lo.W, NC)
    S64, _ = R.reference([dict(maps=maps, size=(HI, WI), crop=(HI, WI), stride=(HI, WI), flip=0)], HI, WI)
    in_band = int(R.tie_band(S64).sum())
    for crop in ((HI, WI), 512):
        c1, m1 = engine.evaluate_msf_slide(_args(hip_graph=False), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10, None, scales=(1.0,), flip=False,
                                           crop=crop)
        moved = int((m1.hist.cpu() - m0.hist.cpu()).abs().sum().item()) // 2
        print(f'[msf-slide e2e] crop {crop}: {moved} pixels counted elsewhere than evaluate, tie band {in_band} pixels')
        assert m1.hist.sum() == m0.hist.sum() and c1.mat.sum() == c0.mat.sum() and m0.hist.sum() > 0
        assert moved <= in_band
        # on this input no pixel of the band flips: the matrices are evaluate's exactly (33 pixels in the band, 0 moved on the MI355X)
        assert torch.equal(m1.hist.cpu(), m0.hist.cpu()) and torch.equal(c1.mat.cpu(), c0.mat.cpu())
    assert not torch.equal(m0.hist.cpu(), e2e.hist)


def test_e2e_predictions_against_float64(e2e):
    sets = [dict(maps=rows.view(2, -1, h, w, NC).cpu(), size=size, crop=crop, stride=stride, flip=f)
            for ((rows, h, w), size, crop, stride), f in zip(e2e.sets, e2e.flips)]
    S64, e32 = R.reference(sets, HI, WI)
    band = R.tie_band(S64)
    print(f'[msf-slide e2e] e32 {e32:.3e} tie band {band.float().mean().item():.4%}')
    assert band.float().mean().item() <= R.TIE_SHARE
    assert torch.equal(e2e.pred[~band], S64.argmax(1)[~band])


def test_semseg_predict_msf_slide(e2e):
    """SemSeg.predict(msf_slide=(crop, stride), scales=, flip=): the kernel's pred_out of the manual path on the preprocessed image."""
    from segmentation_factory_amd import hip
    from segmentation_factory_amd.inference import SemSeg
    ss = SemSeg(e2e.model, img_size=96)
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (3, 96, 160), generator=g, dtype=torch.uint8)
    seg, col = ss.predict(img, overlay=False, msf_slide=(CROP, STRIDE), scales=(0.5, 1.0), flip=True)
    assert seg.shape == (96, 160) and seg.dtype == torch.int64 and col is None
    x = ss.preprocess(img)
    assert tuple(x.shape[2:]) == (96, 160)
    with torch.inference_mode():
        sets, flips = _manual_sets(e2e.model, x, (0.5, 1.0), True)
        pred = torch.empty((1, 96, 160), dtype=torch.int64, device='cuda')
        hip.msf_slide_argmax_confmat(sets, flips, 1, NC, 96, 160, None, 255, None, None, None, pred_out=pred)
    assert torch.equal(seg, pred[0])
    slide, _ = ss.predict(img, overlay=False, slide=(CROP, STRIDE))
    msf, _ = ss.predict(img, overlay=False, scales=(0.5, 1.0), flip=True)
    assert slide.shape == seg.shape and not torch.equal(slide, seg) and msf.shape == seg.shape and not torch.equal(msf, seg)
    small, _ = ss.predict(img[:, :50, :70], overlay=False, msf_slide=(CROP, None), scales=(0.5, 1.0), flip=True)     # original != network size
    assert small.shape == (50, 70) and int(small.min()) >= 0 and int(small.max()) < NC
    with pytest.raises(ValueError):
        ss.predict(img, slide=(CROP, STRIDE), msf_slide=(CROP, STRIDE))
