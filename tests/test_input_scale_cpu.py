"""Scale + padded-crop augmentation of the device input pipeline, host side (no GPU): the draws of
DeviceTrainTransform.draw_scaled follow the reference's call order (datasets/extra_transform.py:90, 359-360, 470-497, 205-213), the
pad rule is extra_transform.py:378-385, the numpy reference of tests/input_scale_refs.py equals Pillow bit for bit on every case
of the shared table, the table covers every padding branch, the command line parses, and nothing changes without the new
arguments."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import input_scale_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated_draws(r, src_h, src_w, size, lo, hi):
    """The composed transforms' draws on `r`, written out from the cited lines."""
    th, tw = size
    scale = r.uniform(lo, hi)                                                     # ExtRandomScale.__call__, :90
    h, w = int(src_h * scale), int(src_w * scale)                                 # :91 (target_size = (h, w))
    P = 0
    if w < tw:                                                                    # :378-380
        pad = int((1 + tw - w) / 2)
        h, w, P = h + 2 * pad, w + 2 * pad, P + pad
    if h < th:                                                                    # :383-385
        pad = int((1 + th - h) / 2)
        h, w, P = h + 2 * pad, w + 2 * pad, P + pad
    if w == tw and h == th:                                                       # get_params, :356-357
        i, j = 0, 0
    else:
        i = r.randint(0, abs(h - th))                                             # :359
        j = r.randint(0, abs(w - tw))                                             # :360
    b, c, s = r.uniform(0.5, 1.5), r.uniform(0.5, 1.5), r.uniform(0.5, 1.5)       # :477, :481, :485
    ops = [(1, b), (2, c), (3, s)]
    r.shuffle(ops)                                                                # :492
    flip = r.random() < 0.5                                                       # :211
    return dict(scale=scale, res_h=int(src_h * scale), res_w=int(src_w * scale), P=P, top=i - P, left=j - P, ops=ops, flip=flip)


@pytest.mark.parametrize('seed', [0, 1, 7, 77, 123])
def test_draw_scaled_follows_the_reference_call_order(seed):
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    t = DeviceTrainTransform((32, 40), device='cpu', rng=random.Random(seed), scale_range=(0.5, 2.0), pad_if_needed=True, label_fill=255)
    r = random.Random(seed)
    for (h, w) in ((37, 53), (64, 48), (96, 130), (20, 20), (33, 90)):
        got = t.draw_scaled(h, w)
        want = _restated_draws(r, h, w, (32, 40), 0.5, 2.0)
        assert got.pop('label_fill') == 255
        assert got == want
    assert t.rng.random() == r.random()                                           # the stream is where the reference's would be


def test_draw_scaled_makes_no_crop_draw_when_the_padded_size_equals_the_crop():
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    # scale exactly 1.0: 20 x 26 -> width pad int((1 + 32 - 26) / 2) = 3 -> 26 x 32; height pad int((1 + 32 - 26) / 2) = 3 -> 32 x 38: draws;
    # 32 x 32 at scale 1.0 fits exactly: no draw; 30 x 30: pad 1 on every side -> 32 x 32: no draw, origin (-1, -1)
    t = DeviceTrainTransform(32, device='cpu', rng=random.Random(5), scale_range=(1.0, 1.0), pad_if_needed=True)
    r = random.Random(5)
    for (h, w), want_p, draws in (((32, 32), 0, False), ((30, 30), 1, False), ((20, 26), 6, True)):
        got = t.draw_scaled(h, w)
        want = _restated_draws(r, h, w, (32, 32), 1.0, 1.0)
        assert got['P'] == want_p == want['P']
        if not draws:
            assert (got['top'], got['left']) == (-want_p, -want_p)
        assert {k: got[k] for k in want} == want
    assert t.rng.random() == r.random()
    # the same three images with a generator that is one randint pair short would differ: the no-draw cases really drew nothing
    r2 = random.Random(5)
    r2.uniform(1.0, 1.0)
    first = [r2.uniform(0.5, 1.5) for _ in range(3)]
    t2 = DeviceTrainTransform(32, device='cpu', rng=random.Random(5), scale_range=(1.0, 1.0), pad_if_needed=True)
    assert sorted(f for _, f in t2.draw_scaled(32, 32)['ops']) == sorted(first)


def test_pad_geometry_hand_table():
    """(res_h, res_w, H, W) -> total border P, by hand from extra_transform.py:378-385 (F.pad with an int pads all four sides)."""
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    table = [
        ((40, 50, 32, 32), 0),        # nothing short
        ((40, 31, 32, 32), 1),        # width short by 1: int(2 / 2) = 1
        ((40, 30, 32, 32), 1),        # by 2: int(3 / 2) = 1 -> 32
        ((40, 29, 32, 32), 2),        # by 3: int(4 / 2) = 2 -> 33 (one more than needed)
        ((29, 40, 32, 32), 2),        # height only
        ((18, 26, 32, 32), 7),        # width: int(7 / 2) = 3 -> 24 x 32; height short by 8: int(9 / 2) = 4 -> total 7
        ((10, 31, 32, 32), 11),       # width pad 1 -> 12 x 33; height short by 20: int(21 / 2) = 10
        ((20, 26, 32, 32), 6),        # 3, then 26 -> short by 6 -> 3
        ((30, 10, 24, 40), 15),       # width short by 30: 15 -> 60 x 40: the width pad already cured the height
        ((1, 1, 32, 32), 16),         # int(32 / 2) = 16 -> 33 x 33
    ]
    for (rh, rw, th, tw), want in table:
        assert DeviceTrainTransform.pad_border(rh, rw, th, tw) == want, (rh, rw, th, tw)
        assert R.pad_border(rh, rw, th, tw)[0] == want
        assert rh + 2 * want >= th and rw + 2 * want >= tw


def test_case_table_covers_every_branch():
    cs = R.CASES
    assert len(cs) == len(R.SOURCES) * len(R.CROPS) * len(R.SCALES)
    assert {(c['src'], c['size'], c['scale']) for c in cs} == {(s, z, f) for s in range(len(R.SOURCES)) for z in R.CROPS for f in R.SCALES}
    assert any(c['P'] == 0 for c in cs), 'no padding'
    assert any(c['by_w'] and not c['by_h'] for c in cs), 'padding by width only'
    assert any(c['by_h'] and not c['by_w'] for c in cs), 'padding by height only'
    assert any(c['by_w'] and c['by_h'] for c in cs), 'padding by both'
    assert any(d % 2 for c in cs for d in c['diffs']), 'an odd size difference'
    assert any(c['top'] < 0 and c['left'] < 0 for c in cs), 'negative top with negative left'
    assert {c['flip'] for c in cs} == {False, True} and {c['label_fill'] for c in cs} == {0, 255}
    orders = {tuple(op for op, _ in c['ops']) for c in cs}
    import itertools
    assert set(itertools.permutations((1, 2, 3))) <= orders and any(2 not in o for o in orders)
    assert any(z[1] % 4 for z in R.CROPS) and any(z[1] % 4 == 0 for z in R.CROPS)
    assert not np.array_equal(R.LUT, np.arange(256))
    for c in cs:                                             # the window lies inside the padded image
        assert 0 <= c['i'] <= c['res_h'] + 2 * c['P'] - c['size'][0] and 0 <= c['j'] <= c['res_w'] + 2 * c['P'] - c['size'][1]


def test_reference_equals_pillow_on_every_case():
    pytest.importorskip('PIL')
    from PIL import Image, ImageOps
    for c in R.CASES:
        img, lbl = R.source(c['src'])
        th, tw = c['size']
        x = Image.fromarray(img).resize((c['res_w'], c['res_h']), Image.BILINEAR)          # F.resize(img, (h, w), BILINEAR)
        y = Image.fromarray(lbl).resize((c['res_w'], c['res_h']), Image.NEAREST)
        if c['P']:
            x = ImageOps.expand(x, border=c['P'], fill=0)                                  # F.pad(img, int): all four borders
            y = ImageOps.expand(y, border=c['P'], fill=c['label_fill'])
        box = (c['j'], c['i'], c['j'] + tw, c['i'] + th)                                   # F.crop(img, i, j, h, w)
        wx, wy = R.scaled_crop(img, lbl, c['res_h'], c['res_w'], c['P'], c['i'], c['j'], c['size'], c['label_fill'])
        assert np.array_equal(np.array(x.crop(box)), wx), c['n']
        assert np.array_equal(np.array(y.crop(box)), wy), c['n']


def test_scaled_record_layout_matches_the_c_compiler(tmp_path):
    from segmentation_factory_amd import hip
    st, name = hip.InputScaledSample, 'segf_input_scaled_sample'
    assert C.sizeof(st) == 80 and C.sizeof(hip.InputSample) == 72
    assert [f for f, _ in st._fields_] == ['img', 'lbl', 'img_stride', 'lbl_stride', 'src_h', 'src_w', 'res_h', 'res_w', 'top', 'left',
                                           'flip', 'order', 'factor', 'label_fill']
    lines = [f'printf("%zu\\n", sizeof({name}));']
    expect = [str(C.sizeof(st))]
    for field, _ in st._fields_:
        lines.append(f'printf("{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
        expect.append(f'{field} {getattr(st, field).offset} {getattr(st, field).size}')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "segfac.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0;\n}\n')
    cc = '/opt/rocm/llvm/bin/clang' if os.path.isfile('/opt/rocm/llvm/bin/clang') else 'cc'
    subprocess.run([cc, '-std=c11', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout
    assert out.split('\n')[:-1] == expect
    assert {'segf_input_train_scaled', 'segf_input_train_scaled_ws'} <= set(hip.exported_symbols())
    for (a, b) in ((37, 18), (53, 26), (64, 64), (48, 96), (2048, 1024), (683, 341)):      # 2 * ceil(max(1, in / out)) + 1
        assert hip.resample_ksize(a, b) == 2 * -(-max(a, b) // b) + 1


def test_cli_flags_parse_and_need_device_input():
    import train_gpu
    base = ['--dataset', 'synthetic']
    p = train_gpu.get_args_parser()
    a = p.parse_args(base + ['--device-input', '--aug-scale', '0.5', '2.0'])
    assert a.aug_scale == [0.5, 2.0] and a.aug_pad_label is None
    train_gpu.check_aug_args(a)
    assert a.aug_pad_label == a.ignore_label == 255                      # padding must not train as class 0
    a = p.parse_args(base + ['--device-input', '--aug-scale', '0.75', '1.5', '--aug-pad-label', '0', '--ignore_label', '200'])
    train_gpu.check_aug_args(a)
    assert a.aug_pad_label == 0
    a = p.parse_args(base + ['--device-input'])
    train_gpu.check_aug_args(a)
    assert a.aug_scale is None                                           # no default: nothing changes
    with pytest.raises(SystemExit, match='--device-input'):
        train_gpu.check_aug_args(p.parse_args(base + ['--aug-scale', '0.5', '2.0']))
    with pytest.raises(SystemExit):
        train_gpu.check_aug_args(p.parse_args(base + ['--device-input', '--aug-scale', '2.0', '0.5']))
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--device-input', '--aug-scale', '0.5'])    # two numbers


def test_default_transform_is_unchanged():
    """Without the new arguments: the four-value draw order as before (crop row, crop column, jitter, flip), the 72-byte record."""
    from segmentation_factory_amd import hip
    from segmentation_factory_amd.transforms import DeviceTrainTransform
    t = DeviceTrainTransform(32, device='cpu', rng=random.Random(9))
    assert t.scale_range is None and not t.pad_if_needed and not t.scaled
    r = random.Random(9)
    for (h, w) in ((50, 60), (32, 32), (20, 45)):
        if (h, w) == (32, 32):
            top, left = 0, 0
        else:
            top, left = r.randint(0, abs(h - 32)), r.randint(0, abs(w - 32))
        ops = [(1, r.uniform(0.5, 1.5)), (2, r.uniform(0.5, 1.5)), (3, r.uniform(0.5, 1.5))]
        r.shuffle(ops)
        flip = r.random() < 0.5
        assert t.draw(h, w) == (top, left, ops, flip)
    assert t.rng.random() == r.random()
    assert C.sizeof(hip.InputSample) == 72
    with pytest.raises(ValueError):
        DeviceTrainTransform(32, device='cpu', scale_range=(0.0, 1.0))
    with pytest.raises(ValueError):
        DeviceTrainTransform(32, device='cpu', scale_range=(0.5, 2.0), label_fill=256)
