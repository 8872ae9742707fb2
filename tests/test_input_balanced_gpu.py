"""Class-balanced crop choice of the device input pipeline on the GPU (csrc/input.hip: segf_input_crop_select,
segf_input_train_scaled_select): `chosen` equals tests/input_balanced_refs.py (the rule the long way round with numpy, pinned against
Pillow and a hand table by tests/test_input_balanced_cpu.py) for every sample, exactly, on both stacks; the batch is the batch of the
plain entry point at the chosen windows, bit for bit."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import input_balanced_refs as R
import input_scale_refs as S

pytestmark = pytest.mark.gpu

OPS = [(1, 1.25), (2, 0.75), (3, 1.5)]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared sources are read-only arrays)


def _transform(size, scaled, lut=R.LUT, **kw):
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    if scaled:
        kw.setdefault('scale_range', (0.5, 2.0))
        kw.setdefault('pad_if_needed', True)
    kw.setdefault('ignore_class', R.IGNORE)
    return DeviceTrainTransform(size, label_lut=None if lut is None else torch.from_numpy(lut), **kw)


def _scaled_params(res, wins, fill, flip=False, ops=OPS):
    return dict(scale=None, res_h=res[0], res_w=res[1], P=0, top=wins[0][0], left=wins[0][1], ops=ops, flip=flip, label_fill=fill,
                windows=list(wins))


def _blocks(h, w, seed, bh=23, bw=31, ncls=4):
    """A piecewise-constant label map (bh x bw blocks of a few classes, 3 % raw 255, some raw 7 beside raw 3)."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, ncls, (h // bh + 1, w // bw + 1)) + 2
    lbl = np.kron(coarse, np.ones((bh, bw), dtype=np.int64))[:h, :w]
    lbl[rng.random((h, w)) < 0.03] = 255
    lbl[(lbl == 3) & (rng.random((h, w)) < 0.3)] = 7
    return lbl.astype(np.uint8)


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize('scaled', [False, True])
def test_hand_table(scaled):
    """The ten rows of the hand table in ONE call (K = 4; 8 x 16 windows of 24 x 40 sources); on the scaled stack at scale 1 with a
    fill of raw 0, which is what Image.crop reads outside the source."""
    t = _transform(R.HAND_SIZE, scaled, lut=R.HAND_LUT, cat_max_ratio=R.HAND_RATIO, crop_tries=3, ignore_class=R.HAND_IGNORE)
    imgs = [_dev(_image(24, 40, 1))] * len(R.HAND)
    lbls = [_dev(lbl) for _, lbl, _, _ in R.HAND]
    if scaled:
        params = [_scaled_params((24, 40), wins, 0) for _, _, wins, _ in R.HAND]
    else:
        params = [(list(wins), OPS, False) for _, _, wins, _ in R.HAND]
    t(imgs, lbls, params)
    assert t.last_chosen.dtype == torch.int32 and t.last_chosen.is_cuda
    assert t.last_chosen.tolist() == [want for _, _, _, want in R.HAND]


@pytest.fixture(scope='module')
def dev_sources():
    return [tuple(_dev(a) for a in S.source(si)) for si in range(len(S.SOURCES))]


@pytest.mark.parametrize('size', S.CROPS)
@pytest.mark.parametrize('stack', ['scaled', 'plain'])
def test_shared_table(stack, size, dev_sources):
    """Every case of one crop size and one stack in ONE call: samples of mixed sources, scales and paddings.  The ratio is an
    argument of the call and differs by case, so there is one call per ratio over ALL the cases, each checked at that call's ratio."""
    idx = [i for i, c in enumerate(R.CASES) if c['stack'] == stack and c['size'] == size]
    cases = [R.CASES[i] for i in idx]
    assert len(cases) >= 6
    imgs, lbls = [dev_sources[c['src']][0] for c in cases], [dev_sources[c['src']][1] for c in cases]
    for ratio in sorted({c['ratio'] for c in cases}):
        t = _transform(size, stack == 'scaled', cat_max_ratio=ratio, crop_tries=R.K - 1)
        if stack == 'scaled':
            params = [_scaled_params(c['res'], c['windows'], c['label_fill'], c['flip'], c['ops']) for c in cases]
        else:
            params = [(c['windows'], c['ops'], c['flip']) for c in cases]
        t(imgs, lbls, params)
        got = t.last_chosen.tolist()
        for k, (i, c) in enumerate(zip(idx, cases)):
            if c['ratio'] == ratio:
                assert got[k] == R.expected(i)[0], (i, c['n'], ratio, c['windows'], R.expected(i))
            else:
                want = R.choose(S.source(c['src'])[1], c['windows'], size, ratio, c['res'], c['label_fill'])[0]
                assert got[k] == want, (i, c['n'], ratio, c['windows'])


@pytest.mark.parametrize('size', [(9, 10), (8, 16)])
@pytest.mark.parametrize('scaled', [False, True])
def test_mixed_batch_unaligned_sources(scaled, size):
    """One call, five samples of mixed sizes (scales and pads on the scaled stack), drawn by the product's own draw functions;
    sub-views with odd row strides and start offsets of every byte alignment."""
    t = _transform(size, scaled, rng=random.Random(31), label_fill=255, cat_max_ratio=0.6, crop_tries=4)
    srcs = [(37, 53), (20, 91), (64, 48), (15, 17), (96, 130)]
    imgs, lbls, host = [], [], []
    for k, (h, w) in enumerate(srcs):
        a = _image(h, w + 3, 50 + k)
        l = np.ascontiguousarray(np.pad(_blocks(h, w, 60 + k, 4, 5, 3), ((0, 0), (k % 4, 5 - k % 4)), constant_values=9))
        da, dl = _dev(a), _dev(l)
        imgs.append(da[:, (k % 3):(k % 3) + w])                     # row stride 3 * (w + 3), start offset 0 / 3 / 6 bytes
        lbls.append(dl[:, (k % 4):(k % 4) + w])                     # row stride w + 5, start offset 0 .. 3 bytes
        host.append(l[:, (k % 4):(k % 4) + w])
    params = [t.draw_scaled(h, w) if scaled else t.draw_balanced(h, w) for (h, w) in srcs]
    geo = [(p['windows'], (p['res_h'], p['res_w']), p['label_fill']) if scaled else (p[0], None, 0) for p in params]
    # the call's ratio: the median share of all tested windows, so that windows pass and fail
    shares = sorted(v for k, (wins, res, fill) in enumerate(geo) for v in R._shares(host[k], wins, size, res, fill))
    ratio = (shares[len(shares) // 2 - 1] + shares[len(shares) // 2]) / 2
    t = _transform(size, scaled, cat_max_ratio=ratio, crop_tries=4)
    t(imgs, lbls, params)
    want = [R.choose(host[k], wins, size, ratio, res, fill)[0] for k, (wins, res, fill) in enumerate(geo)]
    assert t.last_chosen.tolist() == want
    assert len(set(want)) > 1, want


@pytest.mark.parametrize('scaled', [False, True])
def test_the_batch_is_the_old_batch(scaled, dev_sources):
    """A balanced call = the plain entry point with the windows forced to the chosen ones, and the launch trace shows the selection
    kernel in the first call only; with cat_max_ratio=None in neither."""
    from segmentation_factory_amd import hip
    size = (24, 40)
    cases = [c for c in R.CASES if c['stack'] == ('scaled' if scaled else 'plain') and c['size'] == size]
    imgs, lbls = [dev_sources[c['src']][0] for c in cases], [dev_sources[c['src']][1] for c in cases]
    t = _transform(size, scaled, cat_max_ratio=0.3, crop_tries=R.K - 1)
    if scaled:
        params = [_scaled_params(c['res'], c['windows'], c['label_fill'], c['flip'], c['ops']) for c in cases]
    else:
        params = [(c['windows'], c['ops'], c['flip']) for c in cases]
    with hip.trace() as tr1:
        img1, lbl1 = t(imgs, lbls, params)
    chosen = t.last_chosen.tolist()
    assert len(set(chosen)) > 1
    if scaled:
        forced = [dict(p, top=p['windows'][k][0], left=p['windows'][k][1], windows=None) for p, k in zip(params, chosen)]
    else:
        forced = [(p[0][k][0], p[0][k][1], p[1], p[2]) for p, k in zip(params, chosen)]
    with hip.trace() as tr2:
        img2, lbl2 = t(imgs, lbls, forced)
    assert torch.equal(img1, img2) and torch.equal(lbl1, lbl2)
    assert t.last_chosen.tolist() == [0] * len(cases)
    off = _transform(size, scaled)
    for p in forced:
        if scaled:
            p.pop('windows')
    with hip.trace() as tr3:
        img3, lbl3 = off(imgs, lbls, forced)
    assert torch.equal(img1, img3) and torch.equal(lbl1, lbl3) and off.last_chosen is None
    name = 'input_scale_select_kernel' if scaled else 'input_crop_select_kernel'
    assert sum(name in k for k in tr1.kernels) == 1 and tr1.kernels[0].startswith(name)
    assert not any('select' in k for k in tr2.kernels + tr3.kernels)
    assert tr2.kernels == tr3.kernels == tr1.kernels[1:]


def _walk_case(size, scaled, B, K, scales, src_hw=(150, 170), seed=17):
    """B samples = the distinct draws of one block-label source repeated; -> (transform, images, labels, params, expected)."""
    h, w = src_hw
    lbl, img = _blocks(h, w, seed), _image(h, w, seed + 1)
    r = random.Random(seed)
    distinct, want = [], []
    for n, s in enumerate(scales):
        d = _transform(size, scaled, rng=r, scale_range=(s, s) if scaled else None, label_fill=255, cat_max_ratio=0.5, crop_tries=K - 1)
        p = d.draw_scaled(h, w) if scaled else d.draw_balanced(h, w)
        wins, res = (p['windows'], (p['res_h'], p['res_w'])) if scaled else (p[0], None)
        assert len(wins) == K
        distinct.append((p, wins, res))
    # one ratio for the whole call: the median of every tested window's share, so that windows pass and fail
    shares = sorted(v for p, wins, res in distinct for v in R._shares(lbl, wins, size, res, 255))
    ratio = (shares[len(shares) // 2 - 1] + shares[len(shares) // 2]) / 2 if len(shares) > 1 else 0.5
    for p, wins, res in distinct:
        want.append(R.choose(lbl, wins, size, ratio, res, 255)[0])
    t = _transform(size, scaled, cat_max_ratio=ratio, crop_tries=max(K - 1, 1))
    reps = B // len(distinct)
    return t, [_dev(img)] * B, [_dev(lbl)] * B, [p for p, _, _ in distinct] * reps, want * reps


@pytest.mark.parametrize('size', [(264, 264), (131, 131)])
@pytest.mark.parametrize('scaled', [False, True])
def test_batch_of_64_past_one_pass_of_the_workgroup(scaled, size):
    """264 * 17 and 131 * 9 sixteen-pixel segments per window: several passes of the 1024 threads, the last one partly empty; 64
    samples = eight distinct draws, each eight times."""
    assert size[0] * -(-size[1] // 16) > 1024
    src = (300, 340) if not scaled else (150, 170)
    t, imgs, lbls, params, want = _walk_case(size, scaled, 64, 5, (0.5, 0.9, 1.3, 1.6, 1.77, 1.8, 2.0, 2.0), src)
    t(imgs, lbls, params)
    assert t.last_chosen.tolist() == want
    assert len(set(want)) > 1, want


@pytest.mark.parametrize('K', [1, 11, 32])
@pytest.mark.parametrize('scaled', [False, True])
def test_one_sample_and_the_ends_of_K(scaled, K):
    """B = 1 with K = 1 (chosen 0, no label read: the labels are not even consulted), K = 11 (the default) and K = 32 (the most)."""
    from segmentation_factory_amd import hip
    size = (32, 32)
    if K == 1:
        t = _transform(size, scaled, cat_max_ratio=0.5)
        lbl, img = _blocks(60, 70, 3), _image(60, 70, 4)
        chosen = torch.full((1,), -5, dtype=torch.int32, device='cuda')
        if scaled:
            recs, kmax = t.pack_scaled([_dev(img)], [_dev(lbl)], [_scaled_params((60, 70), [(4, 6)], 255)])
            hip.input_train_scaled_select(recs, (C.c_int32 * 2)(4, 6), 1, 1, 32, 32, kmax, 0.5, 255, t.mean, t.std, t.label_lut, chosen=chosen)
        else:
            samples, cand = t.pack([_dev(img)], [_dev(lbl)], [(0, 0, OPS, False)], [4, 6])
            assert hip.input_crop_select(samples, cand, 1, 1, 32, 32, 0.5, t.label_lut, 255, chosen=chosen) is chosen
            rec = hip.InputSample.from_buffer_copy(bytes(samples.cpu().numpy()))
            assert (rec.top, rec.left) == (4, 6)
        assert chosen.tolist() == [0]
        return
    # every tested window but the one at index K - 3 holds a single class, and all of them are DISTINCT (a repeated window is not
    # counted again): the walk counts K - 2 windows, zeroing its counters and passing its barriers each time
    lbl = np.full((120, 130), 2, np.uint8)
    lbl[70:, 80:] = 5
    single = [(k % 38, k) for k in range(K - 1)]             # rows < 70: class 2 only
    wins = single[:K - 3] + [(54, 66), (1, 1), (2, 2)]       # (54, 66): 16 x 18 = 288 pixels of class 5, 736 / 1024 of class 2
    assert len(set(single)) == K - 1
    t = _transform(size, scaled, cat_max_ratio=0.75, crop_tries=K - 1)
    params = [_scaled_params((120, 130), wins, 255)] if scaled else [(wins, OPS, False)]
    t([_dev(_image(120, 130, 5))], [_dev(lbl)], params)
    assert R.choose(lbl, wins, size, 0.75)[0] == K - 3
    assert t.last_chosen.tolist() == [K - 3]
    wins = single + [(54, 66)]                               # none of K - 1 distinct windows passes: K - 1, untested
    params = [_scaled_params((120, 130), wins, 255)] if scaled else [(wins, OPS, False)]
    t([_dev(_image(120, 130, 5))], [_dev(lbl)], params)
    assert R.choose(lbl, wins, size, 0.75)[0] == K - 1
    assert t.last_chosen.tolist() == [K - 1]


def test_sample_without_a_choice_in_a_batch_that_has_one():
    """A source of the crop's size beside a larger one: its one window is repeated, tested once, and reported as index 0 even when
    it fails; the other sample is unaffected."""
    size = (32, 32)
    one = np.full((32, 32), 4, np.uint8)                     # a single class: the window fails
    lbl = np.full((120, 130), 2, np.uint8)
    lbl[70:, 80:] = 5
    wins = [(0, 0), (1, 1), (54, 66), (2, 2), (3, 3)]
    t = _transform(size, False, cat_max_ratio=0.75, crop_tries=4)
    img, out = t([_dev(_image(32, 32, 1)), _dev(_image(120, 130, 2))], [_dev(one), _dev(lbl)], [([(0, 0)], OPS, False), (wins, OPS, True)])
    assert t.last_chosen.tolist() == [0, 2]
    assert torch.equal(out[0].cpu(), torch.from_numpy(R.LUT[one])) and torch.equal(out[1].cpu(), torch.from_numpy(R.LUT[lbl[54:86, 66:98][:, ::-1]].copy()))
    with pytest.raises(ValueError):
        t([_dev(_image(120, 130, 2))], [_dev(lbl)], [([(0, 0)] * 4 + [((1 << 30) + 1, 0)], OPS, False)])


@pytest.mark.parametrize('scale', [0.2, 2.0])
def test_strong_reduction_and_enlargement(scale, dev_sources):
    """Scale 0.2 of the 96 x 130 source (every fifth label, 11 taps in the image path) and 2.0 of the 37 x 53 one."""
    si = 2 if scale < 1 else 0
    size = (24, 40)
    lbl = S.source(si)[1]
    r = random.Random(23)
    d = _transform(size, True, rng=r, scale_range=(scale, scale), label_fill=255, cat_max_ratio=0.5, crop_tries=4)
    params = [d.draw_scaled(*S.SOURCES[si]) for _ in range(3)]
    shares = sorted(v for p in params for v in R._shares(lbl, p['windows'], size, (p['res_h'], p['res_w']), 255))
    ratio = (shares[len(shares) // 2 - 1] + shares[len(shares) // 2]) / 2
    want = [R.choose(lbl, p['windows'], size, ratio, (p['res_h'], p['res_w']), 255)[0] for p in params]
    t = _transform(size, True, cat_max_ratio=ratio, crop_tries=4)
    img, out_lbl = t([dev_sources[si][0]] * 3, [dev_sources[si][1]] * 3, params)
    assert t.last_chosen.tolist() == want
    for k, p in enumerate(params):                           # and the batch is the reference's at the chosen window
        top, left = p['windows'][want[k]]
        c = dict(p, i=top + p['P'], j=left + p['P'], size=size)
        wi, wl = S.scaled_train_transform(*S.source(si), c, label_lut=R.LUT)
        assert torch.equal(out_lbl[k].cpu(), torch.from_numpy(wl)) and torch.equal(img[k].cpu(), torch.from_numpy(wi)), (k, p)


def test_host_refusals_leave_everything_untouched(dev_sources):
    from segmentation_factory_amd import hip
    H = W = 32
    di, dl = dev_sources[2]
    st = torch.cuda.current_stream().cuda_stream
    chosen = torch.full((1,), -5, dtype=torch.int32, device='cuda')
    out_img = torch.full((1, 3, H, W), 123.0, dtype=torch.float32, device='cuda')
    out_lbl = torch.full((1, H, W), -7, dtype=torch.int64, device='cuda')
    # unscaled stack
    t = _transform((H, W), False, cat_max_ratio=0.5, crop_tries=4)
    samples, cand = t.pack([di], [dl], [(3, 4, OPS, False)], [3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    before = samples.clone()

    def plain(K=5, ratio=0.5, h=H, w=W, s=samples.data_ptr(), c=cand.data_ptr()):
        hip._chk_arg(hip.lib().segf_input_crop_select(s, c, 1, K, h, w, ratio, t.label_lut.data_ptr(), 255, chosen.data_ptr(), st),
                     'segf_input_crop_select')
    with hip.trace() as tr:
        for bad in (dict(K=0), dict(K=33), dict(K=-1), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.5), dict(ratio=float('nan')),
                    dict(s=None), dict(c=None), dict(h=32769, w=32769), dict(s=samples.data_ptr() + 8)):
            with pytest.raises(ValueError):
                plain(**bad)
    assert tr.launches == 0 and tr.kernels == []
    # scaled stack
    ts = _transform((H, W), True, cat_max_ratio=0.5, crop_tries=4)
    wins = [(-2, -3), (0, 0), (5, 6), (7, 8), (9, 10)]
    good = _scaled_params((48, 65), wins, 255)
    ws = torch.zeros(int(hip.lib().segf_input_train_scaled_select_ws(1, H, W, 7, 5)) + 16, dtype=torch.uint8, device='cuda')

    def scaled(params=good, K=5, ratio=0.5, kmax=7, h=H, w=W, windows=wins, **over):
        recs, _ = ts.pack_scaled([di], [dl], [params])
        flat = [v for win in windows for v in win]
        a = dict(samples=C.cast(recs, C.c_void_p), cand=C.cast((C.c_int32 * len(flat))(*flat), C.c_void_p), ws=ws.data_ptr(),
                 mean3=ts.mean.data_ptr(), std3=ts.std.data_ptr(), out_img=out_img.data_ptr(), out_lbl=out_lbl.data_ptr())
        a.update(over)
        rc = hip.lib().segf_input_train_scaled_select(a['samples'], a['cand'], K, ratio, 255, chosen.data_ptr(), 1, h, w, kmax, a['ws'],
                                                      a['mean3'], a['std3'], ts.label_lut.data_ptr(), a['out_img'], a['out_lbl'], st)
        hip._chk_arg(rc, 'segf_input_train_scaled_select')
    big = (1 << 30) + 1
    with hip.trace() as tr:
        for bad in (dict(K=0), dict(K=33), dict(ratio=0.0), dict(ratio=1.0001), dict(ratio=float('nan')), dict(samples=None),
                    dict(cand=None), dict(ws=None), dict(mean3=None), dict(std3=None), dict(out_img=None), dict(out_lbl=None),
                    dict(h=32769, w=32769), dict(ws=ws.data_ptr() + 4), dict(kmax=3), dict(params=dict(good, res_h=0)),
                    dict(windows=wins[:4] + [(big, 0)]), dict(windows=wins[:4] + [(0, -big)]), dict(windows=[(-big, 0)] + wins[1:])):
            with pytest.raises(ValueError):
                scaled(**bad)
        with pytest.raises(ValueError):                      # through the Python surface as well
            ts([di], [dl], [dict(good, res_w=0)], out=(out_img, out_lbl))
    assert tr.launches == 0 and tr.kernels == []
    torch.cuda.synchronize()
    assert bool((out_img == 123.0).all()) and bool((out_lbl == -7).all()) and chosen.tolist() == [-5] and torch.equal(samples, before)
    scaled()                                                 # and the same calls, unbroken, work
    plain()
    torch.cuda.synchronize()
    assert 0 <= chosen.tolist()[0] <= 4 and not bool((out_lbl == -7).any())


def _loader_labels(h, w, k):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + 11 * k) // 45 + (xx + 7 * k) // 50) % 5).astype(np.uint8)


def test_zero_copy_feed_of_balanced_batches_into_the_captured_step():
    """DeviceBatchLoader with a balanced (and scaled) transform and bind_output: the yielded buffers are the captured step's static
    inputs, they hold the reference's batch for the same generator state, and a replayed step changes the parameters."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from segmentation_factory_amd.transforms import DeviceBatchLoader, DeviceDataset, DeviceTrainTransform
    ds, host = DeviceDataset(), []
    for k in range(6):
        a, l = _image(60 + 7 * k, 75, 30 + k), _loader_labels(60 + 7 * k, 75, k)
        host.append((a, l))
        ds.add(a, l)

    def make_loader():
        tf = DeviceTrainTransform(64, rng=random.Random(11), scale_range=(0.5, 2.0), pad_if_needed=True, label_fill=255,
                                  cat_max_ratio=0.75, crop_tries=10, ignore_class=255)
        return DeviceBatchLoader(ds, 2, tf, shuffle=True, seed=5)
    model = SegmentationModel('MiT-B0', num_classes=7, seg_head='SegFormerHead', compute_dtype=torch.bfloat16).cuda()
    model.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', 7, 7))
    model.train()
    opt = FusedAGCAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    loader = make_loader()
    seen, losses, picks = [], [], []

    class Rec:
        def add_scalar(self, name, v, it=None):
            if name == 'train_loss':
                gs = model._graphed_step
                seen.append((gs.static_inputs[0].clone(), gs.static_inputs[1].clone()))
                picks.append(loader.transform.last_chosen.tolist())
                losses.append(float(v))
    args = types.SimpleNamespace(nb_classes=7, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)
    engine.train_one_epoch(model, opt, loader, 0, 'cuda', 1, 0.02, 'agc', NativeScaler(), Rec(), args)
    gs = model._graphed_step
    assert loader.out is not None and loader.out[0].data_ptr() == gs.static_inputs[0].data_ptr() \
        and loader.out[1].data_ptr() == gs.static_inputs[1].data_ptr()
    assert len(seen) == 3 and all(np.isfinite(losses))
    ref = make_loader()
    order = ref.indices()
    want_picks = []
    for b, (si, sl) in enumerate(seen):
        for k, idx in enumerate(order[2 * b:2 * b + 2]):
            p = ref.transform.draw_scaled(*host[idx][0].shape[:2])
            pick = R.choose(host[idx][1], p['windows'], (64, 64), 0.75, (p['res_h'], p['res_w']), 255, lut=None, ignore=255)[0]
            want_picks.append(pick)
            top, left = p['windows'][pick]
            c = dict(p, i=top + p['P'], j=left + p['P'], size=(64, 64))
            wi, wl = S.scaled_train_transform(host[idx][0], host[idx][1], c, label_lut=None)
            assert torch.equal(sl[k].cpu(), torch.from_numpy(wl)), (b, k)
            assert torch.equal(si[k].cpu(), torch.from_numpy(wi)), (b, k)
    assert [v for pk in picks for v in pk] == want_picks
    bi, bl = next(iter(loader))
    assert bi.data_ptr() == gs.static_inputs[0].data_ptr() and bl.data_ptr() == gs.static_inputs[1].data_ptr()
    before = [p.detach().clone() for p in model.parameters()]
    gs.step(bi, bl)
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_train_gpu_cli_with_aug_cat_max_ratio(tmp_path):
    """train_gpu.py --device-input --aug-scale 0.5 2.0 --aug-cat-max-ratio 0.75: one short epoch at 64 x 64 in a fresh child
    process, finite loss."""
    import glob
    import math
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'train_gpu.py'), '--dataset', 'synthetic', '--data_len', '8', '--image_size', '64',
           '--nb_classes', '5', '--backbone', 'MiT-B0', '--heads', 'SegFormerHead', '--batch-size', '4', '--val_batch_size', '2',
           '--epochs', '1', '--save_weights_dir', str(tmp_path / 'out'), '--writer_output', str(tmp_path), '--train_print_freq', '1',
           '--val_print_freq', '1', '--lr', '2e-3', '--device-input', '--aug-scale', '0.5', '2.0', '--aug-cat-max-ratio', '0.75']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'aug_cat_max_ratio=0.75' in r.stdout and 'aug_crop_tries=10' in r.stdout
    res = glob.glob(str(tmp_path / 'results*.txt'))
    assert res, r.stdout[-2000:]
    losses = [float(v) for v in re.findall(r'train_loss: ([0-9.naninf]+)', open(res[0]).read())]
    assert len(losses) == 1 and math.isfinite(losses[0]), losses
