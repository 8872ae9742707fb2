"""Sliding-window evaluation on the GPU: segf_slide_argmax_confmat (csrc/eval_slide.hip) against the float64 torch restatement of
tests/slide_refs.py, and engine.evaluate_slide / Metrics.update_slide / SemSeg.predict(slide=...) on top of it.

Mean logits: mean_out against oracle(float64) within atol = max(4 e32, 16 n_max 2^-24 M) -- e32 = the error of oracle(float32) against
oracle(float64) on the same inputs, n_max the largest cover count, M the largest input magnitude (derivation: slide_refs.atol_of; the
figures seen on the MI355X are recorded in profiles/slide_eval.md).  The geometry 16, 16 / 9, 9 / 3, 3 has FOUR windows per axis
(origins 0, 3, 6, 7), i.e. a 16-fold cover; it is kept under the same formula next to a true 9-fold one (15, 15 / 9, 9 / 3, 3).
Predictions: equal to the float64 arg max wherever the float64 top-2 margin is at least 2 atol; the pixels inside that band are at
most 0.5 % (asserted on the reference alone, first).  Counts: equal to a bincount of (target, pred_out) on ALL pixels, which checks the
counting independently of ties."""
import types

import pytest
import torch

import slide_refs as R

pytestmark = pytest.mark.gpu

STORAGE = [torch.float32, torch.bfloat16]
B = 2

# name -> (H, W, crop, stride, (h, w), C, ldl padding, seed).  The seed is one at which the reference-only tie-band condition holds
# for both storages: on maps this small two bf16 logits of one pixel can be EQUAL, which puts every pixel that reads only that tap
# into the band.
GEOMS = {
    'one-window': (8, 8, (8, 8), (8, 8), (2, 2), 19, 0, 0),
    'shifted-last-window': (8, 14, (8, 8), (8, 5), (2, 2), 19, 0, 0),
    'grid-2x3': (20, 29, (12, 16), (8, 9), (3, 4), 19, 3, 0),         # columns 0, 9, 13: 3-fold across, 2-fold down
    'cover-9': (15, 15, (9, 9), (3, 3), (3, 3), 19, 0, 1),            # origins 0, 3, 6 per axis
    'cover-16': (16, 16, (9, 9), (3, 3), (3, 3), 19, 0, 0),           # origins 0, 3, 6, 7 per axis: rows / columns 7, 8 lie in all four
    'stride==crop': (10, 10, (4, 4), (4, 4), (1, 1), 19, 0, 0),
    'map>crop': (10, 11, (4, 4), (3, 3), (6, 6), 19, 0, 0),
    'map==crop': (11, 13, (5, 6), (3, 5), (5, 6), 19, 3, 1),
    'C2': (20, 29, (12, 16), (8, 9), (3, 4), 2, 0, 0),
    'C65': (20, 29, (12, 16), (8, 9), (3, 4), 65, 0, 2),
    'C150': (20, 29, (12, 16), (8, 9), (3, 4), 150, 3, 2),
    'C192': (20, 29, (12, 16), (8, 9), (3, 4), 192, 0, 1),
}
N_MAX = {'one-window': 1, 'shifted-last-window': 3, 'grid-2x3': 6, 'cover-9': 9, 'cover-16': 16, 'stride==crop': 4, 'map>crop': 4,
         'map==crop': 4}


def _case(name, storage):
    H, W, crop, stride, hw, C, pad, seed = GEOMS[name]
    return (H, W, crop, stride, hw, C, pad), R.case(C, H, W, crop, stride, hw, storage, B=B, seed=seed)


def _check(name, storage, ref, out):
    """The numerical bar of one kernel result against the shared reference; the figures are printed before the assertions."""
    err = (out['mean'].double() - ref['M64'].permute(0, 2, 3, 1)).abs().max().item()
    share = ref['band'].float().mean().item()
    wrong = ((out['pred'] != ref['M64'].argmax(1)) & ~ref['band']).sum().item()
    print(f'[slide {name} {storage}] n_max {ref["n_max"]} M {ref["M"]:.2f} e32 {ref["e32"]:.3e} atol {ref["atol"]:.3e} '
          f'kernel err {err:.3e} tie band {share:.4%} wrong outside the band {wrong}')
    assert err <= ref['atol'], (name, err, ref['atol'])
    assert wrong == 0


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(GEOMS))
def test_mean_predictions_and_counts(name, storage):
    (H, W, crop, stride, hw, C, pad), ref = _case(name, storage)
    assert ref['band'].float().mean().item() <= R.TIE_SHARE              # a condition on the reference, before the kernel is looked at
    if name in N_MAX:
        assert ref['n_max'] == N_MAX[name]
    target = R.make_target(B, H, W, C)
    out = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=target, ldl=C + pad)
    _check(name, storage, ref, out)
    mat, hist = R.counts(target, out['pred'], C, 255)
    assert torch.equal(out['mat'], mat) and torch.equal(out['hist'], hist) and out['flag'] == 0
    assert out['hist'].sum().item() == (target != 255).sum().item() > 0
    if name == 'C65':
        assert (out['pred'] >= 64).any()                               # the second slot wins somewhere
    if name in ('C150', 'C192'):
        assert (out['pred'] >= 128).any()                              # and the third


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
def test_singly_covered_pixels_keep_their_sample(storage):
    """Division by n = 1 is exact: where one window covers a pixel, mean_out is that window's sample -- the one-window call on that
    window's map -- bit for bit."""
    (H, W, crop, stride, hw, C, pad), ref = _case('grid-2x3', storage)
    out = R.run_kernel(ref['maps'], C, H, W, crop, stride)
    _, _, origins = R.windows_of(H, W, crop, stride)
    once = ref['cnt'] == 1
    assert once.any()
    for k, (y, x) in enumerate(origins):
        single = R.run_kernel(ref['maps'][:, k:k + 1].contiguous(), C, crop[0], crop[1], crop, crop)['mean']
        m = once[y:y + crop[0], x:x + crop[1]]
        assert torch.equal(out['mean'][:, y:y + crop[0], x:x + crop[1]][:, m], single[:, m])


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
def test_one_window_reduces_to_argmax_confmat(storage):
    """One window that is the whole image: predictions and counts are segf_argmax_confmat's on the same map."""
    from segmentation_factory_amd import hip
    (H, W, crop, stride, (h, w), C, pad), ref = _case('one-window', storage)
    target = R.make_target(B, H, W, C)
    out = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=target)
    mat = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.empty((B, H, W), dtype=torch.int64, device='cuda')
    hip.argmax_confmat(ref['maps'].reshape(B * h * w, C).cuda(), B, C, h, w, H, W, target.cuda(), 255, mat, hist, flag, pred)
    assert torch.equal(out['pred'], pred.cpu())
    assert torch.equal(out['mat'], mat.cpu()) and torch.equal(out['hist'], hist.cpu()) and out['mat'].sum() > 0


@pytest.mark.parametrize('storage', STORAGE, ids=['f32', 'bf16'])
@pytest.mark.parametrize('ignore_label,bad_label', [(3, None), (255, 200), (255, -3)], ids=['ignore-in-range', 'bad-label', 'negative-label'])
def test_counting_rule(ignore_label, bad_label, storage):
    (H, W, crop, stride, hw, C, pad), ref = _case('grid-2x3', storage)
    target = R.make_target(B, H, W, C, ignore_label, bad_label)
    out = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=target, ignore_label=ignore_label)
    _check('grid-2x3 counting', storage, ref, out)
    mat, hist = R.counts(target, out['pred'], C, ignore_label)
    assert torch.equal(out['mat'], mat) and torch.equal(out['hist'], hist)
    in_range = (target >= 0) & (target < C)
    assert out['mat'].sum().item() == in_range.sum().item()
    assert out['hist'].sum().item() == (in_range & (target != ignore_label)).sum().item()
    assert out['flag'] == (1 if bad_label is not None else 0)       # the bad label is flagged and (sums above) counted nowhere
    if 0 <= ignore_label < C:
        assert out['mat'][ignore_label].sum() > 0 and out['hist'][ignore_label].sum() == 0


def test_counting_alone_skips_nothing_it_must_count():
    """Without pred_out / mean_out the kernel skips pixels that are counted nowhere: the counts are those of the full call."""
    (H, W, crop, stride, hw, C, pad), ref = _case('grid-2x3', torch.bfloat16)
    target = R.make_target(B, H, W, C)
    full = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=target)
    bare = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=target, want_pred=False, want_mean=False)
    assert torch.equal(full['mat'], bare['mat']) and torch.equal(full['hist'], bare['hist']) and bare['hist'].sum() > 0


def test_no_target_means_no_counting():
    (H, W, crop, stride, hw, C, pad), ref = _case('grid-2x3', torch.float32)
    out = R.run_kernel(ref['maps'], C, H, W, crop, stride, target=None, mat_fill=7)
    assert bool((out['mat'] == 7).all()) and bool((out['hist'] == 7).all()) and out['flag'] == 0
    _check('grid-2x3 no target', torch.float32, ref, out)
    assert int(out['pred'].min()) >= 0


def test_two_runs_give_the_same_bits():
    for name in ('cover-9', 'C150'):
        (H, W, crop, stride, hw, C, pad), ref = _case(name, torch.bfloat16)
        a = R.run_kernel(ref['maps'], C, H, W, crop, stride)
        b = R.run_kernel(ref['maps'], C, H, W, crop, stride)
        assert torch.equal(a['mean'], b['mean']) and torch.equal(a['pred'], b['pred'])


def test_layout_mismatches_raise():
    from segmentation_factory_amd import hip
    rows = torch.zeros((2 * 6 * 12, 19), device='cuda')
    pred = torch.empty((2, 20, 29), dtype=torch.int64, device='cuda')
    hip.slide_argmax_confmat((rows, 3, 4), 2, 19, 20, 29, (12, 16), (8, 9), None, 255, None, None, None, pred_out=pred)
    with pytest.raises(ValueError):                                   # one window short
        hip.slide_argmax_confmat((rows[:-12], 3, 4), 2, 19, 20, 29, (12, 16), (8, 9), None, 255, None, None, None, pred_out=pred)
    with pytest.raises(ValueError):                                   # fewer columns than classes
        hip.slide_argmax_confmat((rows[:, :18], 3, 4), 2, 19, 20, 29, (12, 16), (8, 9), None, 255, None, None, None, pred_out=pred)
    with pytest.raises(ValueError):                                   # inner stride 2
        hip.slide_argmax_confmat((torch.zeros((144, 38), device='cuda')[:, ::2], 3, 4), 2, 19, 20, 29, (12, 16), (8, 9), None, 255, None,
                                 None, None, pred_out=pred)
    with pytest.raises(ValueError):                                   # stride larger than the crop
        hip.slide_argmax_confmat((rows, 3, 4), 2, 19, 20, 29, (12, 16), (13, 9), None, 255, None, None, None, pred_out=pred)


# ---- end to end: MiT-B0 + SegFormerHead, B = 2, 96 x 160, crop 64, stride 48 (a 2 x 3 grid) ---------------------------------------
NC, HI, WI, CROP, STRIDE = 7, 96, 160, 64, 48


@pytest.fixture(scope='module')
def e2e():
    """Model, batch and the manual loop's result (one forward_lowres per window, one update_slide), computed once."""
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, engine, hip, utils
    from segmentation_factory_amd.metrics import Metrics
    model = SegmentationModel('MiT-B0', num_classes=NC, seg_head='SegFormerHead', compute_dtype=torch.float32)
    model.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', NC, 77, lively=True))
    model = model.cuda().eval()
    x, y = OW.synthetic_batch(2, HI, WI, NC, 78)                     # labels with an ignored band and ~2 % ignored pixels
    x, y = x.cuda(), y.cuda()
    crop, stride, origins = engine.slide_windows(HI, WI, CROP, STRIDE)
    assert crop == (64, 64) and stride == (48, 48) and origins == [(0, 0), (0, 48), (0, 96), (32, 0), (32, 48), (32, 96)]
    with torch.inference_mode():
        per = []                                                       # [image][window] -> rows [h*w, >= NC]
        for b in range(2):
            per.append([])
            for (oy, ox) in origins:
                lo = model.forward_lowres(x[b:b + 1, :, oy:oy + 64, ox:ox + 64].contiguous())
                assert (lo.B, lo.H, lo.W) == (1, 16, 16)
                per[b].append(lo.data[:, :NC].clone())
        rows = torch.cat([r for img in per for r in img]).contiguous()

        def count(r):
            metric, confmat = Metrics(NC, 255, 'cuda'), utils.ConfusionMatrix(NC)
            metric.update_slide((r, 16, 16), y, (HI, WI), CROP, STRIDE, confmat=confmat)
            return metric.hist.cpu().clone(), confmat.mat.cpu().clone()
        hist, mat = count(rows)
        pred = torch.empty((2, HI, WI), dtype=torch.int64, device='cuda')
        hip.slide_argmax_confmat((rows, 16, 16), 2, NC, HI, WI, CROP, STRIDE, None, 255, None, None, None, pred_out=pred)
        # the aliasing trap is visible on this input: with window_batch = 4 the 12 windows travel as 3 chunks of 4; were every chunk
        # read from one static buffer after the last replay, all three would hold the last chunk's result
        chunks = rows.view(3, 4 * 256, NC)
        aliased_hist, _ = count(chunks[2:3].expand(3, -1, -1).reshape(-1, NC).contiguous())
        stale_hist, _ = count(torch.cat([chunks[0], chunks[0], chunks[1]]).contiguous())       # each chunk one replay late
    assert not torch.equal(aliased_hist, hist) and not torch.equal(stale_hist, hist)
    return types.SimpleNamespace(model=model, x=x, y=y, rows=rows, origins=origins, hist=hist, mat=mat, pred=pred.cpu())


def _args(**kw):
    return types.SimpleNamespace(nb_classes=NC, ignore_label=255, **kw)


@pytest.mark.parametrize('window_batch', [None, 4, 5], ids=['all', 'chunks-of-4', 'chunks-of-5'])
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_evaluate_slide_matches_the_manual_loop(e2e, graph, window_batch):
    """The loader yields the same batch twice.  With the graph on, a chunk shape is captured on its second sighting and replayed from
    then on, every chunk of that shape out of ONE static output buffer: the aliasing trap.  Both sightings must add the manual loop's
    counts, whatever the chunking (5 does not divide the 12 windows: a remainder chunk of another shape)."""
    from segmentation_factory_amd import engine
    confmat, metric = engine.evaluate_slide(_args(hip_graph=graph), e2e.model, [(e2e.x, e2e.y)] * 2, 'cuda', 10, None, crop=CROP,
                                            stride=STRIDE, window_batch=window_batch)
    assert e2e.hist.sum() > 0
    assert torch.equal(metric.hist.cpu(), 2 * e2e.hist)
    assert torch.equal(confmat.mat.cpu(), 2 * e2e.mat)


def test_crop_of_the_image_size_is_evaluate(e2e):
    """Crop >= image size: one window = the whole image, so the counts are evaluate's, exactly."""
    from segmentation_factory_amd import engine
    c0, m0 = engine.evaluate(_args(hip_graph=False), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    for crop in ((HI, WI), 512):
        c1, m1 = engine.evaluate_slide(_args(hip_graph=False), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10, None, crop=crop)
        assert torch.equal(m1.hist.cpu(), m0.hist.cpu()) and torch.equal(c1.mat.cpu(), c0.mat.cpu())
    assert m0.hist.sum() > 0 and not torch.equal(m0.hist.cpu(), e2e.hist)          # sliding windows are a different prediction


def test_evaluate_dispatches_on_eval_mode(e2e, monkeypatch):
    from segmentation_factory_amd import engine
    a = _args(hip_graph=False, eval_mode='slide', eval_crop=[CROP], eval_stride=[STRIDE], eval_window_batch=4)
    confmat, metric = engine.evaluate(a, e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert torch.equal(metric.hist.cpu(), e2e.hist) and torch.equal(confmat.mat.cpu(), e2e.mat)
    # crop from image_size, stride floor(2 crop / 3) = 42: another grid (2 x 4), hence other counts than stride 48
    assert len(engine.slide_windows(HI, WI, 64, engine.default_slide_stride(64))[2]) == 8
    confmat, metric = engine.evaluate(_args(hip_graph=False, eval_mode='slide', image_size=64), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert metric.hist.sum() == e2e.hist.sum() and not torch.equal(metric.hist.cpu(), e2e.hist)
    # without the mode (absent, or the CLI's default) evaluate_slide is not called
    def boom(*a, **k):
        raise AssertionError('evaluate_slide was called')
    monkeypatch.setattr(engine, 'evaluate_slide', boom)
    c0, m0 = engine.evaluate(_args(hip_graph=False), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    c1, m1 = engine.evaluate(_args(hip_graph=False, eval_mode='whole', eval_crop=[CROP]), e2e.model, [(e2e.x, e2e.y)], 'cuda', 10)
    assert torch.equal(m0.hist.cpu(), m1.hist.cpu()) and m0.hist.sum() > 0


def test_e2e_predictions_against_float64(e2e):
    maps = e2e.rows.view(2, 6, 16, 16, NC).cpu()
    M64, cnt = R.oracle(maps, HI, WI, (CROP, CROP), (STRIDE, STRIDE), torch.float64)
    M32, _ = R.oracle(maps, HI, WI, (CROP, CROP), (STRIDE, STRIDE), torch.float32)
    e32 = (M32.double() - M64).abs().max().item()
    atol = R.atol_of(e32, int(cnt.max()), maps.abs().max().item())
    band = R.tie_band(M64, atol)
    print(f'[slide e2e] n_max {int(cnt.max())} e32 {e32:.3e} atol {atol:.3e} tie band {band.float().mean().item():.4%}')
    assert band.float().mean().item() <= R.TIE_SHARE
    assert torch.equal(e2e.pred[~band], M64.argmax(1)[~band])


def test_semseg_predict_slide(e2e):
    """SemSeg.predict(slide=(crop, stride)): the kernel's pred_out of the manual path on the preprocessed image."""
    from segmentation_factory_amd import engine, hip
    from segmentation_factory_amd.inference import SemSeg
    ss = SemSeg(e2e.model, img_size=96)
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (3, 96, 160), generator=g, dtype=torch.uint8)
    seg, col = ss.predict(img, overlay=False, slide=(CROP, STRIDE))
    assert seg.shape == (96, 160) and seg.dtype == torch.int64 and col is None
    x = ss.preprocess(img)
    assert tuple(x.shape[2:]) == (96, 160)
    _, _, origins = engine.slide_windows(96, 160, CROP, STRIDE)
    with torch.inference_mode():
        rows = torch.cat([e2e.model.forward_lowres(x[:, :, oy:oy + 64, ox:ox + 64].contiguous()).data[:, :NC] for oy, ox in origins])
        pred = torch.empty((1, 96, 160), dtype=torch.int64, device='cuda')
        hip.slide_argmax_confmat((rows.contiguous(), 16, 16), 1, NC, 96, 160, CROP, STRIDE, None, 255, None, None, None, pred_out=pred)
    assert torch.equal(seg, pred[0])
    plain, _ = ss.predict(img, overlay=False)
    assert plain.shape == seg.shape and not torch.equal(plain, seg)
    small, _ = ss.predict(img[:, :50, :70], overlay=False, slide=(CROP, None))       # original size != network input size
    assert small.shape == (50, 70) and int(small.min()) >= 0 and int(small.max()) < NC
    with pytest.raises(ValueError):
        ss.predict(img, slide=(CROP, STRIDE), flip=True)
    with pytest.raises(ValueError):
        ss.predict(img, slide=(CROP, STRIDE), scales=(0.5, 1.0))
