"""Reference of the class-balanced crop choice for the tests of the device input pipeline (test infrastructure, not a test module).

The rule (include/segfac.h, segf_input_crop_select) restates mmsegmentation's RandomCrop(crop_size, cat_max_ratio): draw a window; up
to ten times, crop the label map, `np.unique(labels, return_counts=True)`, drop the ignore index, and stop when
`len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < cat_max_ratio`, else draw again; the window drawn after the last failed test is used
untested.  Here it is written the long way round with numpy: the WHOLE label map is resized (oracle.input_pipeline.resize_nearest),
padded with np.pad and the fill, cropped (oracle.input_pipeline.crop), sent through the label table, counted with np.unique.

CASES is the one table that the CPU and the GPU tests share: tests/input_scale_refs.SOURCES x CROPS x SCALES, K = 5 windows each,
for the scaled stack and (at the source's own size, no padding) for the unscaled one.
"""
import random

import numpy as np

import input_scale_refs as S
from oracle import input_pipeline as IP

IGNORE = 255                                                 # 5 % of every source is raw 255
K = 5
LUT = np.arange(256, dtype=np.int64)
LUT[7] = 3                                                   # raw 3 and raw 7 are one class; a pad fill of 0 is class 0, counted


def window_labels(lbl, top, left, size, res=None, label_fill=0):
    """The raw uint8 labels of one window.  res=None: the unscaled stack, Image.crop at (top, left) of the source (0 outside).
    res=(res_h, res_w): the scaled stack, (top, left) in RESIZED coordinates: resize everything, pad by as much as the window needs
    with `label_fill`, crop."""
    th, tw = size
    if res is None:
        return IP.crop(lbl, top, left, th, tw)
    y = IP.resize_nearest(lbl, res[0], res[1])
    P = max(0, -top, -left, top + th - res[0], left + tw - res[1])
    if P:
        y = np.pad(y, ((P, P), (P, P)), constant_values=label_fill)
    return IP.crop(y, top + P, left + P, th, tw)


def verdict(raw, ratio, lut=LUT, ignore=IGNORE):
    """-> (passes, why) for one window of raw labels; why in {'pass', 'one_class', 'ratio'}."""
    cls = raw.astype(np.int64) if lut is None else np.asarray(lut, np.int64)[raw]
    labels, cnt = np.unique(cls, return_counts=True)
    cnt = cnt[labels != ignore]
    if not len(cnt) > 1:
        return False, 'one_class'
    if cnt.max() / cnt.sum() < ratio:
        return True, 'pass'
    return False, 'ratio'


def choose(lbl, windows, size, ratio, res=None, label_fill=0, lut=LUT, ignore=IGNORE):
    """mmseg's loop over the candidate list: the first len(windows) - 1 are tested, the last is taken as it comes.
    -> (chosen index, [why of every tested window])."""
    whys = []
    for k, (top, left) in enumerate(windows[:-1]):
        ok, why = verdict(window_labels(lbl, top, left, size, res, label_fill), ratio, lut, ignore)
        whys.append(why)
        if ok:
            return k, whys
    return len(windows) - 1, whys


def _shares(lbl, windows, size, res, label_fill):
    """max_c n_c / sum_c n_c of every tested window that holds more than one class."""
    out = []
    for top, left in windows[:-1]:
        cls = LUT[window_labels(lbl, top, left, size, res, label_fill)]
        labels, cnt = np.unique(cls, return_counts=True)
        cnt = cnt[labels != IGNORE]
        if len(cnt) > 1:
            out.append(cnt.max() / cnt.sum())
    return sorted(out)


def _ratio(shares, mode):
    """A ratio that lets a different number of the windows pass: above every share (mode 0), between two neighbouring shares
    (1 .. 3), below every share (4: none passes)."""
    if not shares:
        return 0.5
    if mode == 0:
        return (shares[-1] + 1.0) / 2
    if mode == 4 or len(shares) == 1:
        return shares[0] * 0.9
    j = min(mode, len(shares) - 1)
    return (shares[j - 1] + shares[j]) / 2


def _make_cases():
    cases = []
    for c in S.CASES:
        n = c['n']
        r = random.Random(7000 + n)
        (h, w), (th, tw) = S.SOURCES[c['src']], c['size']
        lbl = S.source(c['src'])[1]
        hp, wp = c['res_h'] + 2 * c['P'], c['res_w'] + 2 * c['P']
        wins = [(r.randint(0, abs(hp - th)) - c['P'], r.randint(0, abs(wp - tw)) - c['P']) for _ in range(K)]
        if n % 4 == 1 and c['P']:                            # a window whose corner lies in the border
            wins[1] = (-c['P'], -c['P'])
        if n % 6 == 2:                                       # a window of nothing but the fill: one class, or none at all
            wins[0] = (-th - 3, c['res_w'] + 2)
        res = (c['res_h'], c['res_w'])
        cases.append(dict(n=n, stack='scaled', src=c['src'], size=c['size'], res=res, P=c['P'], windows=wins,
                          label_fill=c['label_fill'], ratio=_ratio(_shares(lbl, wins, c['size'], res, c['label_fill']), n % 5),
                          scale=c['scale'], ops=c['ops'], flip=c['flip']))
        if c['scale'] in (1.0, 2.0):                         # the unscaled stack on the same source, twice; windows may hang over the edge
            m = sum(1 for x in cases if x['stack'] == 'plain')
            wins = [(r.randint(0, abs(h - th)), r.randint(0, abs(w - tw))) for _ in range(K)]
            if m % 3 == 0:
                wins[0] = (h, 0)                             # wholly below the source: the raw 0 of Image.crop, one class
            cases.append(dict(n=n, stack='plain', src=c['src'], size=c['size'], res=None, P=0, windows=wins, label_fill=0,
                              ratio=_ratio(_shares(lbl, wins, c['size'], None, 0), m % 5), scale=None, ops=c['ops'], flip=c['flip']))
    return cases


CASES = _make_cases()
_WANT = {}


def expected(i):
    """(chosen, whys) of CASES[i], computed once."""
    if i not in _WANT:
        c = CASES[i]
        _WANT[i] = choose(S.source(c['src'])[1], c['windows'], c['size'], c['ratio'], c['res'], c['label_fill'])
    return _WANT[i]


# ---- the hand table: source 24 x 40, windows 8 x 16 = 128 pixels, K = 4 -------------------------------------------------------------
HAND_SIZE, HAND_RATIO, HAND_IGNORE = (8, 16), 0.75, 255
HAND_LUT = np.arange(256, dtype=np.int64)
HAND_LUT[7] = 3                                              # raw 3 and raw 7 are one class
HAND_LUT[9] = 255                                            # raw 9 lands on the ignore class


def _hand_source(blocks):
    """24 x 40 label map, raw 1 everywhere, then {(top, left): 8 x 16 block}."""
    a = np.full((24, 40), 1, np.uint8)
    for (t, l), blk in blocks.items():
        a[t:t + 8, l:l + 16] = blk
    return a


def _split(n_first, first, second):
    """8 x 16 block whose first n_first pixels (row-major) are `first`, the rest `second`."""
    b = np.full(128, second, np.uint8)
    b[:n_first] = first
    return b.reshape(8, 16)


def _three(n_a, a, n_b, b, rest):
    x = np.full(128, rest, np.uint8)
    x[:n_a] = a
    x[n_a:n_a + n_b] = b
    return x.reshape(8, 16)


A, B_, C_ = (0, 0), (8, 16), (16, 24)                        # three disjoint window origins
# each row: (name, label map, [4 windows], expected chosen) -- worked out by hand, ratio 0.75, ignore 255
HAND = [
    ('first window passes', _hand_source({A: _split(64, 2, 4)}), [A, B_, C_, A], 0),                              # 64 / 64 = 0.5
    ('two single-class windows, then a mixed one', _hand_source({C_: _split(40, 2, 5)}), [A, B_, C_, A], 2),      # 88 / 128
    ('96 / 32 is exactly 0.75 and fails, 95 / 33 passes', _hand_source({A: _split(96, 2, 4), B_: _split(95, 2, 4)}), [A, B_, C_, C_], 1),
    ('all four fail: the last is taken untested', _hand_source({}), [A, B_, C_, (3, 5)], 3),
    ('120 ignored + 4 + 4 passes', _hand_source({A: _three(4, 2, 4, 4, 255)}), [A, B_, C_, C_], 0),               # 4 / 8 = 0.5
    ('120 ignored + 8 of one class fails', _hand_source({A: _three(4, 2, 4, 2, 255), B_: _split(64, 2, 4)}), [A, B_, C_, C_], 1),
    ('an all-ignored window fails', _hand_source({A: _split(128, 255, 255), B_: _split(64, 2, 4)}), [A, B_, C_, C_], 1),
    ('raw 3 and raw 7 are one class', _hand_source({A: _split(64, 3, 7), B_: _three(40, 3, 40, 7, 5)}), [A, B_, C_, C_], 1),   # 80 / 128
    ('a raw value mapped onto the ignore class is not counted', _hand_source({A: _split(64, 9, 2), B_: _three(100, 9, 14, 2, 4)}),
     [A, B_, C_, C_], 1),                                    # window A: 64 of class 2 only; window B: 14 / 28 = 0.5
    # (20, 30): rows 20 .. 23 and columns 30 .. 39 exist: 4 x 10 = 40 pixels of raw 1, 88 zeros from outside: 88 / 128 < 0.75
    ('a window over the source edge counts the raw 0 it reads there', _hand_source({}), [A, (20, 30), C_, C_], 1),
]
