"""Scale + padded-crop augmentation of the device input pipeline on the GPU (csrc/input.hip: segf_input_train_scaled) -- BIT-EXACT
against tests/input_scale_refs.py (resize the whole image the way Pillow does, pad, crop, then the unchanged train stack) over the
case table that tests/test_input_scale_cpu.py pins against Pillow itself: torch.equal on the fp32 image and the int64 label."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import input_scale_refs as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared sources are read-only arrays)


def _transform(size, **kw):
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    kw.setdefault('scale_range', (0.5, 2.0))
    kw.setdefault('pad_if_needed', True)
    return DeviceTrainTransform(size, label_lut=torch.from_numpy(R.LUT), **kw)


@pytest.fixture(scope='module')
def dev_sources():
    return [tuple(_dev(a) for a in R.source(si)) for si in range(len(R.SOURCES))]


@pytest.mark.parametrize('size', R.CROPS)
def test_kernel_bit_exact_over_the_case_table(size, dev_sources):
    cases = [c for c in R.CASES if c['size'] == size]
    assert len(cases) == len(R.SOURCES) * len(R.SCALES)
    t = _transform(size)
    img, lbl = t([dev_sources[c['src']][0] for c in cases], [dev_sources[c['src']][1] for c in cases], [R.as_params(c) for c in cases])
    assert img.shape == (len(cases), 3) + size and img.dtype == torch.float32 and lbl.shape == (len(cases),) + size and lbl.dtype == torch.int64
    img, lbl = img.cpu(), lbl.cpu()
    for k, c in enumerate(cases):
        wi, wl = R.expected(c['n'])
        assert torch.equal(lbl[k], torch.from_numpy(wl)), (c['n'], c['scale'], c['P'], c['top'], c['left'])
        assert torch.equal(img[k], torch.from_numpy(wi)), (c['n'], c['scale'], c['P'], c['top'], c['left'],
                                                           float((img[k] - torch.from_numpy(wi)).abs().max()))


@pytest.mark.parametrize('size', [(32, 32), (30, 30)])
def test_scale_one_ties_to_the_unscaled_path(size):
    """Scale exactly 1.0: a source of the crop's size (window = image), and a larger one cropped at an offset, give the bits of
    segf_input_train on the same parameters."""
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    rng = np.random.default_rng(21)
    plain = DeviceTrainTransform(size, label_lut=torch.from_numpy(R.LUT), rng=random.Random(2))
    scaled = _transform(size, scale_range=(1.0, 1.0))
    imgs, lbls, old, new = [], [], [], []
    for (h, w) in (size, (size[0] + 9, size[1] + 14), size):
        imgs.append(_dev(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        lbls.append(_dev(rng.integers(0, 256, (h, w), dtype=np.uint8)))
        top, left, ops, flip = plain.draw(h, w)
        old.append((top, left, ops, flip))
        new.append(dict(scale=1.0, res_h=h, res_w=w, P=0, top=top, left=left, ops=ops, flip=flip, label_fill=255))
    assert old[0][:2] == (0, 0) and old[1][:2] != (0, 0)
    a = plain(imgs, lbls, old)
    b = scaled(imgs, lbls, new)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_mixed_batch_unaligned_sources():
    """One call, five samples of mixed sizes, scales and pads, drawn by the product's own draw_scaled; sub-views with odd row strides
    and start offsets of every byte alignment."""
    size = (24, 40)
    t = _transform(size, rng=random.Random(31), label_fill=255)
    rng = np.random.default_rng(8)
    srcs = [(37, 53), (20, 91), (64, 48), (15, 17), (96, 130)]
    imgs, lbls, host = [], [], []
    for k, (h, w) in enumerate(srcs):
        a = rng.integers(0, 256, (h, w + 3, 3), dtype=np.uint8)
        l = rng.integers(0, 256, (h, w + 5), dtype=np.uint8)
        da, dl = _dev(a), _dev(l)
        imgs.append(da[:, (k % 3):(k % 3) + w])                     # row stride 3 * (w + 3), start offset 0 / 3 / 6 bytes
        lbls.append(dl[:, (k % 4):(k % 4) + w])
        host.append((a[:, (k % 3):(k % 3) + w], l[:, (k % 4):(k % 4) + w]))
    params = [t.draw_scaled(h, w) for (h, w) in srcs]
    assert len({p['P'] for p in params}) > 1 and any(p['scale'] < 1 for p in params) and any(p['scale'] > 1 for p in params)
    img, lbl = t(imgs, lbls, params)
    img, lbl = img.cpu(), lbl.cpu()
    for k, p in enumerate(params):
        c = dict(p, i=p['top'] + p['P'], j=p['left'] + p['P'], size=size)
        wi, wl = R.scaled_train_transform(host[k][0], host[k][1], c)
        assert torch.equal(lbl[k], torch.from_numpy(wl)), (k, p)
        assert torch.equal(img[k], torch.from_numpy(wi)), (k, p)


@pytest.mark.parametrize('size', [(24, 40), (30, 30)])
def test_strong_reduction_with_nine_and_eleven_taps(size, dev_sources):
    """The case table stops at 7 taps per axis (scale 0.5); below scale 1/3 a pixel has 9 and 11 (here, in both pixel forms),
    and the table rows are kmax = 11 wide for every sample of the batch."""
    from segmentation_factory_amd import hip
    r = random.Random(13)
    params = [_transform(size, rng=r, scale_range=(s, s), label_fill=255).draw_scaled(*R.SOURCES[2]) for s in (0.3, 0.21, 0.3)]
    t = _transform(size)
    recs, kmax = t.pack_scaled([dev_sources[2][0]] * 3, [dev_sources[2][1]] * 3, params)
    assert kmax == 11 and hip.resample_ksize(96, int(96 * 0.3)) == 9
    img, lbl = t([dev_sources[2][0]] * 3, [dev_sources[2][1]] * 3, params)
    for k, p in enumerate(params):
        wi, wl = R.scaled_train_transform(*R.source(2), dict(p, i=p['top'] + p['P'], j=p['left'] + p['P'], size=size))
        assert torch.equal(lbl[k].cpu(), torch.from_numpy(wl)), (k, p)
        assert torch.equal(img[k].cpu(), torch.from_numpy(wi)), (k, p)


@pytest.mark.parametrize('size', [(264, 264), (131, 131)])
def test_batch_of_64_walks_the_grid_stride_loop(size):
    """From batch 64 on the grid is capped at 64 workgroups per sample; with more than 64 * 256 runs per crop every thread takes
    several (4-pixel form: 264 * 66 runs; 1-pixel form: 131 * 131).  Eight distinct draws, each eight times in the batch."""
    assert size[0] * (size[1] // 4 if size[1] % 4 == 0 else size[1]) > 64 * 256
    rng = np.random.default_rng(17)
    a, l = rng.integers(0, 256, (150, 170, 3), dtype=np.uint8), rng.integers(0, 256, (150, 170), dtype=np.uint8)
    r = random.Random(4)
    distinct = [_transform(size, rng=r, scale_range=(s, s), label_fill=255).draw_scaled(150, 170)
                for s in (0.5, 0.9, 1.3, 1.6, 1.77, 1.8, 2.0, 2.0)]
    assert any(p['P'] == 0 for p in distinct) and any(p['P'] > 0 for p in distinct)
    da, dl = _dev(a), _dev(l)
    img, lbl = _transform(size)([da] * 64, [dl] * 64, distinct * 8)
    img, lbl = img.cpu(), lbl.cpu()
    for k, p in enumerate(distinct):
        wi, wl = R.scaled_train_transform(a, l, dict(p, i=p['top'] + p['P'], j=p['left'] + p['P'], size=size))
        wi, wl = torch.from_numpy(wi), torch.from_numpy(wl)
        for rep in range(8):
            assert torch.equal(lbl[k + 8 * rep], wl), (k, rep, p)
            assert torch.equal(img[k + 8 * rep], wi), (k, rep, p)


def test_workspace_does_not_depend_on_the_resized_size(dev_sources):
    from segmentation_factory_amd import hip
    size = (32, 32)
    lo = next(c for c in R.CASES if c['size'] == size and c['scale'] == 0.5 and c['src'] == 2)
    hi = next(c for c in R.CASES if c['size'] == size and c['scale'] == 2.0 and c['src'] == 2)
    t = _transform(size)
    sizes = []
    for c in (lo, hi):
        recs, kmax = t.pack_scaled([dev_sources[2][0]], [dev_sources[2][1]], [R.as_params(c)])
        sizes.append(int(hip.lib().segf_input_train_scaled_ws(1, 32, 32, 7)))
        assert kmax <= 7
        ws = torch.empty(sizes[-1], dtype=torch.uint8, device='cuda')           # the same buffer size serves both
        img, lbl = hip.input_train_scaled(recs, 1, 32, 32, 7, t.mean, t.std, t.label_lut, ws=ws)
        assert torch.equal(img[0].cpu(), torch.from_numpy(R.expected(c['n'])[0])) and torch.equal(lbl[0].cpu(), torch.from_numpy(R.expected(c['n'])[1]))
    assert sizes[0] == sizes[1] > 0
    # tables + two staged uint8 planes: far below a resized image of the larger case would need, and linear in the batch
    assert sizes[0] < 4 * 32 * 32 + 8 * (32 + 32) * (3 + 7) + 1024
    assert int(hip.lib().segf_input_train_scaled_ws(4, 32, 32, 7)) <= 4 * sizes[0]


def test_host_refusals_leave_the_outputs_untouched(dev_sources):
    from segmentation_factory_amd import hip
    H = W = 32
    t = _transform((H, W))
    c = next(c for c in R.CASES if c['size'] == (H, W) and c['scale'] == 0.5 and c['src'] == 2)
    di, dl = dev_sources[2]
    out_img = torch.full((1, 3, H, W), 123.0, dtype=torch.float32, device='cuda')
    out_lbl = torch.full((1, H, W), -7, dtype=torch.int64, device='cuda')
    slack_img = torch.full((3 * H * W + 8,), 123.0, dtype=torch.float32, device='cuda')
    slack_lbl = torch.full((H * W + 4,), -7, dtype=torch.int64, device='cuda')
    ws = torch.zeros(int(hip.lib().segf_input_train_scaled_ws(1, H, W, 7)) + 16, dtype=torch.uint8, device='cuda')

    def call(params=None, kmax=7, h=H, w=W, **over):
        recs, _ = t.pack_scaled([di], [dl], [params or R.as_params(c)])
        a = dict(samples=C.cast(recs, C.c_void_p), ws=ws.data_ptr(), mean3=t.mean.data_ptr(), std3=t.std.data_ptr(),
                 out_img=out_img.data_ptr(), out_lbl=out_lbl.data_ptr())
        a.update(over)
        rc = hip.lib().segf_input_train_scaled(a['samples'], 1, h, w, kmax, a['ws'], a['mean3'], a['std3'], t.label_lut.data_ptr(),
                                               a['out_img'], a['out_lbl'], torch.cuda.current_stream().cuda_stream)
        hip._chk_arg(rc, 'segf_input_train_scaled')

    for name in ('samples', 'ws', 'mean3', 'std3', 'out_img', 'out_lbl'):                    # null pointers
        with pytest.raises(ValueError):
            call(**{name: None})
    with pytest.raises(ValueError):                                                          # misaligned outputs / workspace
        call(out_img=slack_img.data_ptr() + 4)
    with pytest.raises(ValueError):
        call(out_lbl=slack_lbl.data_ptr() + 8)
    with pytest.raises(ValueError):
        call(ws=ws.data_ptr() + 4)
    for bad in (dict(res_h=0), dict(res_w=0), dict(res_h=-3)):
        with pytest.raises(ValueError):
            call(params=dict(R.as_params(c), **bad))
    with pytest.raises(ValueError):                                                          # 96 -> 48 needs 5 taps, 130 -> 65 too
        call(kmax=3)
    with pytest.raises(ValueError):
        call(params=dict(R.as_params(c), res_h=31), kmax=5)                                  # 96 / 31 > 3: 9 taps
    with pytest.raises(ValueError):                                                          # H * W > 2^30
        call(h=32769, w=32769)
    with pytest.raises(ValueError):                                                          # through the Python surface as well
        t([di], [dl], [dict(R.as_params(c), res_w=0)], out=(out_img, out_lbl))
    torch.cuda.synchronize()
    assert bool((out_img == 123.0).all()) and bool((out_lbl == -7).all())
    assert bool((slack_img == 123.0).all()) and bool((slack_lbl == -7).all())
    call()                                                                                   # and the same call, unbroken, works
    assert torch.equal(out_img[0].cpu(), torch.from_numpy(R.expected(c['n'])[0]))
    assert torch.equal(out_lbl[0].cpu(), torch.from_numpy(R.expected(c['n'])[1]))


def test_zero_copy_feed_of_scaled_batches_into_the_captured_step():
    """DeviceBatchLoader with a scaled transform and bind_output: the yielded buffers are the captured step's static inputs, they
    hold the reference's batch for the same generator state, and a replayed step changes the parameters."""
    import types
    from oracle import weights as OW
    from segmentation_factory_amd import SegmentationModel, engine
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler
    from segmentation_factory_amd.transforms import DeviceBatchLoader, DeviceDataset, DeviceTrainTransform
    rng = np.random.default_rng(3)
    ds, host = DeviceDataset(), []
    for k in range(6):
        a, l = rng.integers(0, 256, (60 + 7 * k, 75, 3), dtype=np.uint8), rng.integers(0, 5, (60 + 7 * k, 75), dtype=np.uint8)
        host.append((a, l))
        ds.add(a, l)

    def make_loader():
        tf = DeviceTrainTransform(64, rng=random.Random(11), scale_range=(0.5, 2.0), pad_if_needed=True, label_fill=255)
        return DeviceBatchLoader(ds, 2, tf, shuffle=True, seed=5)
    model = SegmentationModel('MiT-B0', num_classes=5, seg_head='SegFormerHead', compute_dtype=torch.bfloat16).cuda()
    model.load_state_dict(OW.make_state_dict('MiT-B0', 'SegFormerHead', 5, 7))
    model.train()
    opt = FusedAGCAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    loader = make_loader()
    seen, losses = [], []

    class Rec:
        def add_scalar(self, name, v, it=None):
            if name == 'train_loss':
                gs = model._graphed_step
                seen.append((gs.static_inputs[0].clone(), gs.static_inputs[1].clone()))
                losses.append(float(v))
    args = types.SimpleNamespace(nb_classes=5, dice=True, ignore_index=255, ignore_label=255, local_rank=0, device='cuda', hip_graph=True)
    engine.train_one_epoch(model, opt, loader, 0, 'cuda', 1, 0.02, 'agc', NativeScaler(), Rec(), args)
    gs = model._graphed_step
    assert loader.out is not None and loader.out[0].data_ptr() == gs.static_inputs[0].data_ptr() \
        and loader.out[1].data_ptr() == gs.static_inputs[1].data_ptr()
    assert len(seen) == 3 and all(np.isfinite(losses))
    # what the step read = the reference's batches for the same generator state and the same index order
    ref = make_loader()
    order = ref.indices()
    for b, (si, sl) in enumerate(seen):
        for k, idx in enumerate(order[2 * b:2 * b + 2]):
            p = ref.transform.draw_scaled(*host[idx][0].shape[:2])
            c = dict(p, i=p['top'] + p['P'], j=p['left'] + p['P'], size=(64, 64))
            wi, wl = R.scaled_train_transform(host[idx][0], host[idx][1], c, label_lut=None)
            assert torch.equal(sl[k].cpu(), torch.from_numpy(wl)), (b, k)
            assert torch.equal(si[k].cpu(), torch.from_numpy(wi)), (b, k)
    # the bound loader yields the step's own tensors, and one more replayed step moves the parameters
    bi, bl = next(iter(loader))
    assert bi.data_ptr() == gs.static_inputs[0].data_ptr() and bl.data_ptr() == gs.static_inputs[1].data_ptr()
    before = [p.detach().clone() for p in model.parameters()]
    gs.step(bi, bl)
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_train_gpu_cli_with_aug_scale(tmp_path):
    """train_gpu.py --device-input --aug-scale 0.5 2.0: one short epoch at 64 x 64 in a fresh child process, finite loss."""
    import glob
    import math
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'train_gpu.py'), '--dataset', 'synthetic', '--data_len', '8', '--image_size', '64',
           '--nb_classes', '5', '--backbone', 'MiT-B0', '--heads', 'SegFormerHead', '--batch-size', '4', '--val_batch_size', '2',
           '--epochs', '1', '--save_weights_dir', str(tmp_path / 'out'), '--writer_output', str(tmp_path), '--train_print_freq', '1',
           '--val_print_freq', '1', '--lr', '2e-3', '--device-input', '--aug-scale', '0.5', '2.0']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'aug_pad_label=255' in r.stdout                                   # the default follows --ignore_label
    res = glob.glob(str(tmp_path / 'results*.txt'))
    assert res, r.stdout[-2000:]
    losses = [float(v) for v in re.findall(r'train_loss: ([0-9.naninf]+)', open(res[0]).read())]
    assert len(losses) == 1 and math.isfinite(losses[0]), losses
