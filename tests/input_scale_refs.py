"""Reference of the scaled training stack for the tests of the device input pipeline (test infrastructure, not a test module).

    ExtCompose([ExtRandomScale((lo, hi)), ExtRandomCrop((H, W), pad_if_needed=True), ExtColorJitter, ExtRandomHorizontalFlip,
                ExtToTensor, ExtNormalize])                  (datasets/extra_transform.py:75-96, 319-392, 426-509, 196-214, 259-313)
followed by the label table, composed from oracle/input_pipeline.py the long way round: resize the WHOLE image (IP.resize_bilinear /
IP.resize_nearest), np.pad with the fills, crop, IP.train_transform.  torchvision is not installed, so the reference's classes
cannot be executed; the pin is Pillow itself, which those classes call (tests/test_input_scale_cpu.py), plus the cited lines.

CASES is the one table that the CPU and the GPU tests share.
"""
import itertools
import random

import numpy as np

from oracle import input_pipeline as IP

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
LUT = np.arange(256, dtype=np.int64)
LUT[255] = 0
LUT[7] = 3                                                   # a non-identity label table
SOURCES = [(37, 53), (64, 48), (96, 130)]                    # (h, w)
CROPS = [(32, 32), (24, 40), (30, 30)]                       # (H, W); 30: W % 4 != 0
SCALES = [0.5, 0.61, 1.0, 1.37, 2.0]
# every jitter order that contains a contrast step (2), and two without
ORDERS = [list(p) for p in itertools.permutations((1, 2, 3))] + [[2], [1, 2], [3, 2], [1, 3], []]


def pad_border(res_h, res_w, th, tw):
    """extra_transform.py:378-385, restated: F.pad(img, int) pads all four borders; width first, then height on the padded size.
    -> (total border P, padded by width?, padded by height?, the size differences that went through int((1 + d) / 2))."""
    p, by_w, by_h, diffs = 0, False, False, []
    if res_w < tw:
        by_w = True
        diffs.append(tw - res_w)
        p = int((1 + tw - res_w) / 2)
    h = res_h + 2 * p
    if h < th:
        by_h = True
        diffs.append(th - h)
        p += int((1 + th - h) / 2)
    return p, by_w, by_h, diffs


def _make_cases():
    cases = []
    combos = list(itertools.product(range(len(SOURCES)), range(len(CROPS)), SCALES))
    for n, (si, ci, scale) in enumerate(combos):
        (h, w), (th, tw) = SOURCES[si], CROPS[ci]
        r = random.Random(1000 + n)
        res_h, res_w = int(h * scale), int(w * scale)        # extra_transform.py:91
        P, by_w, by_h, diffs = pad_border(res_h, res_w, th, tw)
        hp, wp = res_h + 2 * P, res_w + 2 * P
        if (hp, wp) == (th, tw):
            i = j = 0
        else:
            i, j = r.randint(0, abs(hp - th)), r.randint(0, abs(wp - tw))
        if n % 4 == 1:                                       # the window's corner inside the border whenever there is one
            i, j = min(i, max(P - 1, 0)), min(j, max(P - 1, 0))
        ops = [(op, r.uniform(0.5, 1.5)) for op in ORDERS[n % len(ORDERS)]]
        cases.append(dict(n=n, src=si, size=(th, tw), scale=scale, res_h=res_h, res_w=res_w, P=P, by_w=by_w, by_h=by_h, diffs=diffs,
                          i=i, j=j, top=i - P, left=j - P, ops=ops, flip=bool(n % 2), label_fill=255 if (n // 2) % 2 else 0))
    return cases


CASES = _make_cases()
_SRC = {}


def source(si):
    """The decoded (image uint8 [h, w, 3], label uint8 [h, w]) of SOURCES[si]: generated once, shared, never written to."""
    if si not in _SRC:
        h, w = SOURCES[si]
        rng = np.random.default_rng(40 + si)
        # smooth-ish content plus noise (so that taps matter), labels in blocks with some 255 and 7 (the table's two special values)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(yy * 5 + xx * 3) % 256, (yy * 2 + xx * 7 + 40) % 256, (yy * xx) % 256], -1) + rng.integers(-30, 31, (h, w, 3))
        lbl = ((yy // 5) * 3 + xx // 7) % 11
        lbl[rng.random((h, w)) < 0.05] = 255
        img, lbl = np.clip(img, 0, 255).astype(np.uint8), lbl.astype(np.uint8)
        img.setflags(write=False)
        lbl.setflags(write=False)
        _SRC[si] = (img, lbl)
    return _SRC[si]


def scaled_crop(img, lbl, res_h, res_w, P, i, j, size, label_fill):
    """Resize everything, pad, crop at (i, j) of the PADDED image -> uint8 (crop image [H, W, 3], crop label [H, W])."""
    x, y = IP.resize_bilinear(img, res_h, res_w), IP.resize_nearest(lbl, res_h, res_w)
    if P:
        x = np.pad(x, ((P, P), (P, P), (0, 0)), constant_values=0)
        y = np.pad(y, ((P, P), (P, P)), constant_values=label_fill)
    return IP.crop(x, i, j, size[0], size[1]), IP.crop(y, i, j, size[0], size[1])


def scaled_train_transform(img, lbl, c, mean=MEAN, std=STD, label_lut=LUT):
    """One case through the whole stack -> (float32 [3, H, W], int64 [H, W])."""
    x, y = scaled_crop(img, lbl, c['res_h'], c['res_w'], c['P'], c['i'], c['j'], c['size'], c['label_fill'])
    return IP.train_transform(x, y, dict(top=0, left=0, ops=c['ops'], flip=c['flip']), c['size'], mean, std, label_lut)


_WANT = {}


def expected(n):
    """scaled_train_transform of CASES[n], computed once."""
    if n not in _WANT:
        c = CASES[n]
        _WANT[n] = scaled_train_transform(*source(c['src']), c)
    return _WANT[n]


def as_params(c):
    """CASES entry -> the dict that DeviceTrainTransform.draw_scaled returns."""
    return dict(scale=c['scale'], res_h=c['res_h'], res_w=c['res_w'], P=c['P'], top=c['top'], left=c['left'], ops=c['ops'],
                flip=c['flip'], label_fill=c['label_fill'])
