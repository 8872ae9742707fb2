"""Host side of the sliding-window evaluation (no GPU): the C ABI entries are declared, documented and exported, the window grid of
the library equals engine.slide_windows, every shape the header says is refused is refused before any launch, the class count picks
the kernel form, train_gpu.py has the flags and engine.evaluate refuses the combinations that are not built."""
import ctypes as C
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_DTYPE = -1, -2


def _lib():
    from segmentation_factory_amd import hip
    if not os.path.isfile(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return hip.lib()


def test_header_declares_and_documents_the_entries():
    from segmentation_factory_amd import hip
    header = open(os.path.join(ROOT, 'include', 'segfac.h')).read()
    lib = _lib()
    for name in ('segf_slide_grid', 'segf_slide_supported', 'segf_slide_argmax_confmat'):
        assert name in hip.exported_symbols()
        assert hasattr(lib, name)
    assert re.search(r'#define\s+SEGF_ERR_DTYPE\s+\(?-2\)?', header)
    doc = header[header.index('sliding-window evaluation'):header.index('int segf_slide_grid')]
    doc = ' '.join(re.sub(r'^\s*\*\s', ' ', doc, flags=re.M).split())              # one line, comment margins removed
    assert 'ny = max(H - ch + sh - 1, 0) / sh + 1' in doc and 'y_i = min(i sh, H - ch)' in doc     # the grid formula
    assert 'shifted back' in doc and 'never coincide' in doc
    assert 'added in window order' in doc and 'ascending (i, j) order' in doc and 'same bits' in doc   # the order of the sum
    assert 'true IEEE fp32 division' in doc and 'bit for bit' in doc                # the true division
    assert 'lowest class index' in doc and 'i nx + j' in doc and 'can be captured' in doc
    res, args = hip._DECLS['segf_slide_argmax_confmat']
    assert res is C.c_int and len(args) == 22
    assert len(hip._DECLS['segf_slide_grid'][1]) == 8 and len(hip._DECLS['segf_slide_supported'][1]) == 11


def _grid(H, W, ch, cw, sh, sw):
    ny, nx = C.c_int(-7), C.c_int(-7)
    rc = _lib().segf_slide_grid(H, W, ch, cw, sh, sw, C.byref(ny), C.byref(nx))
    return rc, ny.value, nx.value


def test_grid_equals_slide_windows():
    """Every (H, crop, stride) with H in 1..40 on the row axis against a second, different triple on the column axis: the library's
    counts are engine.slide_windows', whose origins are strictly increasing, end at the border and leave no pixel uncovered."""
    from segmentation_factory_amd import hip
    from segmentation_factory_amd.engine import slide_windows
    triples = [(L, c, s) for L in range(1, 41) for c in range(1, L + 1) for s in range(1, c + 1)]
    n = len(triples)
    for k, (H, ch, sh) in enumerate(triples):
        W, cw, sw = triples[(k * 7919 + 13) % n]
        crop, stride, origins = slide_windows(H, W, (ch, cw), (sh, sw))
        assert crop == (ch, cw) and stride == (sh, sw)
        rc, ny, nx = _grid(H, W, ch, cw, sh, sw)
        assert rc == 0 and ny * nx == len(origins), (H, W, ch, cw, sh, sw)
        ys, xs = [y for y, _ in origins[::nx]], [x for _, x in origins[:nx]]
        assert origins == [(y, x) for y in ys for x in xs] and len(ys) == ny
        for o, L, c, s in ((ys, H, ch, sh), (xs, W, cw, sw)):
            assert o[0] == 0 and o[-1] == L - c and all(b > a and b - a <= s for a, b in zip(o, o[1:]))     # s <= c: no gap
            assert o == [min(i * s, L - c) for i in range(len(o))]
        assert hip.slide_grid(H, W, (ch, cw), (sh, sw)) == (ny, nx)


def test_grid_spot_values():
    from segmentation_factory_amd import hip
    from segmentation_factory_amd.engine import slide_windows
    crop, stride, origins = slide_windows(8, 14, 8, 5)
    assert (crop, stride) == ((8, 8), (5, 5)) and origins == [(0, 0), (0, 5), (0, 6)]
    assert _grid(8, 14, 8, 8, 5, 5) == (0, 1, 3)
    _, _, origins = slide_windows(10, 10, 4, 4)
    assert [x for _, x in origins[:3]] == [0, 4, 6] and [y for y, _ in origins[::3]] == [0, 4, 6] and len(origins) == 9
    assert _grid(10, 10, 4, 4, 4, 4) == (0, 3, 3)
    assert hip.slide_grid(1024, 2048, 1024, 768) == (1, 3) and hip.slide_grid(512, 683, 512, 341) == (1, 2)
    # the crop is clamped to the image and the stride to the crop by engine.slide_windows; the library refuses instead
    assert slide_windows(6, 9, 8, (7, 5)) == ((6, 8), (6, 5), [(0, 0), (0, 1)])
    with pytest.raises(ValueError):
        hip.slide_grid(6, 9, 8, 5)
    with pytest.raises(ValueError):
        slide_windows(6, 9, 0, 1)


GOOD = dict(dt=0, B=2, Cc=19, H=20, W=29, ch=12, cw=16, sh=8, sw=9, h=3, w=4, ldl=19, logits=0x1000, mean=False, ldm=0)


def _call(**kw):
    """Both entries with placeholder device pointers (never dereferenced: every case here is refused before a launch)."""
    a = dict(GOOD, **kw)
    lib = _lib()
    sup = lib.segf_slide_supported(a['dt'], a['B'], a['Cc'], a['H'], a['W'], a['ch'], a['cw'], a['sh'], a['sw'], a['h'], a['w'])
    rc = lib.segf_slide_argmax_confmat(a['dt'], a['B'], a['Cc'], a['H'], a['W'], a['ch'], a['cw'], a['sh'], a['sw'], a['h'], a['w'],
                                       a['logits'], a['ldl'], None, 255, None, None, None, None, 0x2000 if a['mean'] else None, a['ldm'],
                                       None)
    return sup, rc


def test_acceptable_shapes_are_supported():
    lib = _lib()
    assert lib.segf_slide_supported(0, 2, 19, 20, 29, 12, 16, 8, 9, 3, 4) == 1
    assert lib.segf_slide_supported(1, 65535, 192, 1, 1, 1, 1, 1, 1, 1, 1) == 1          # the limits are inclusive
    assert lib.segf_slide_supported(1, 1, 1, 4, 4, 4, 4, 4, 4, 6, 6) == 1                # stride == crop == image, map larger than crop


@pytest.mark.parametrize('kw', [dict(Cc=0), dict(Cc=193), dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(h=0), dict(w=0),
                                dict(sh=0), dict(sw=0), dict(sh=13), dict(sw=17), dict(ch=21), dict(cw=30), dict(ch=0, sh=0),
                                dict(sh=-1), dict(H=11), dict(W=15)],
                         ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_refused_by_both_entries(kw):
    sup, rc = _call(**kw)
    assert sup == 0 and rc == ERR_SHAPE
    a = dict(GOOD, **kw)
    if any(k in kw for k in ('H', 'W', 'ch', 'cw', 'sh', 'sw')):                     # the grid entry refuses the same grids
        assert _grid(a['H'], a['W'], a['ch'], a['cw'], a['sh'], a['sw'])[0] == ERR_SHAPE


@pytest.mark.parametrize('kw', [dict(ldl=18), dict(mean=True, ldm=18), dict(logits=None)], ids=['ldl<C', 'ldm<C', 'logits=NULL'])
def test_refused_by_the_main_entry(kw):
    """Row strides and pointers are not part of segf_slide_supported's signature: the main entry refuses them."""
    sup, rc = _call(**kw)
    assert sup == 1 and rc == ERR_SHAPE


def test_unknown_dtype():
    sup, rc = _call(dt=7)
    assert sup == 0 and rc == ERR_DTYPE
    assert _lib().segf_slide_grid(20, 29, 12, 16, 8, 9, None, None) == ERR_SHAPE


def test_dry_run_reaches_the_kernel_of_each_class_count():
    """One launch per call (dry run: the decision is recorded, nothing runs); the class count picks the lane group (16 / 32 / 64 lanes
    per pixel) and the slots per lane; C = 192 and a padded mean_out are launched."""
    from segmentation_factory_amd import hip
    lib = _lib()
    for Cc, want in ((2, '1, 16>'), (16, '1, 16>'), (19, '1, 32>'), (33, '1, 64>'), (64, '1, 64>'), (65, '2, 64>'), (150, '3, 64>'),
                     (192, '3, 64>')):
        for dt in (0, 1):
            with hip.trace(dry_run=True) as t:
                rc = lib.segf_slide_argmax_confmat(dt, 2, Cc, 20, 29, 12, 16, 8, 9, 3, 4, 0x1000, Cc + 3, None, 255, None, None, None, None,
                                                   0x2000, Cc, None)
            assert rc == 0 and t.launches == 1, (Cc, rc, t.kernels)
            assert 'slide_argmax_confmat_kernel' in t.kernels[0] and want in t.kernels[0].replace('T = ', ''), t.kernels


def _parser():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_gpu_cli_slide', os.path.join(ROOT, 'train_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return argparse.ArgumentParser(parents=[mod.get_args_parser()])


def test_cli_flags():
    from segmentation_factory_amd.engine import default_slide_stride
    parser = _parser()
    args = parser.parse_args([])
    assert args.eval_mode == 'whole' and args.eval_crop is None and args.eval_stride is None and args.eval_window_batch is None
    assert not args.eval_scales and args.eval_flip is False                             # the MSF defaults are untouched
    args = parser.parse_args(['--eval-mode', 'slide', '--eval-crop', '512', '--eval-stride', '341', '--eval-window-batch', '4'])
    assert args.eval_mode == 'slide' and args.eval_crop == [512] and args.eval_stride == [341] and args.eval_window_batch == 4
    args = parser.parse_args(['--eval-mode', 'slide', '--eval-crop', '1024', '2048', '--eval-stride', '768', '1024'])
    assert args.eval_crop == [1024, 2048] and args.eval_stride == [768, 1024]
    with pytest.raises(SystemExit):
        parser.parse_args(['--eval-mode', 'tiles'])
    assert default_slide_stride(512) == (341, 341) and default_slide_stride((1024, 512)) == (682, 341) and default_slide_stride(1) == (1, 1)


class _Stub:
    """A model that must never run: the combinations are refused before any forward."""

    def eval(self):
        return self

    def __call__(self, x):
        raise AssertionError('the model was run')


@pytest.mark.parametrize('kw', [dict(eval_scales=[0.5, 1.0]), dict(eval_flip=True), dict(eval_scales=[1.0], eval_flip=True),
                                dict(eval_scales=[1.5])], ids=['scales', 'flip', 'scale1+flip', 'one-other-scale'])
def test_evaluate_refuses_slide_with_scales_or_flip(kw):
    from segmentation_factory_amd import engine
    args = types.SimpleNamespace(nb_classes=7, ignore_label=255, eval_mode='slide', eval_crop=[64], **kw)
    with pytest.raises(ValueError, match='several scales or mirrored are not built'):
        engine.evaluate(args, _Stub(), [], 'cpu', 10)


def test_evaluate_slide_on_an_empty_loader():
    """eval_mode == 'slide' alone (also with the scale list (1.0,)) reaches evaluate_slide: no batch, empty matrices, no forward."""
    from segmentation_factory_amd import engine
    for kw in (dict(), dict(eval_scales=[1.0], eval_flip=False)):
        args = types.SimpleNamespace(nb_classes=7, ignore_label=255, eval_mode='slide', eval_crop=[64], eval_stride=None, **kw)
        confmat, metric = engine.evaluate(args, _Stub(), [], 'cpu', 10)
        assert float(metric.hist.sum()) == 0.0
