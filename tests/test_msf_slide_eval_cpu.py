"""Host side of the multi-scale + flip sliding-window evaluation (no GPU): the C ABI entries are declared, documented and exported,
refuse what the header says they refuse before any launch, the class count picks the kernel form, train_gpu.py has the mode and
engine.evaluate dispatches on it while the plain slide mode keeps refusing scales and flip."""
import ctypes as C
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_DTYPE = -1, -2
# Hs, Ws, ch, cw, sh, sw, h, w
GOOD_GEOM = [[20, 29, 12, 16, 8, 9, 3, 4], [40, 58, 12, 16, 8, 9, 3, 4]]


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
    for name in ('segf_msf_slide_supported', 'segf_msf_slide_argmax_confmat'):
        assert name in hip.exported_symbols()
        assert hasattr(lib, name)
    doc = header[header.index('multi-scale + flip SLIDING-WINDOW'):header.index('int segf_msf_slide_supported')]
    doc = ' '.join(re.sub(r'^\s*\*\s', ' ', doc, flags=re.M).split())              # one line, comment margins removed
    assert 'Hs_k, Ws_k' in doc and 'ch_k, cw_k' in doc and 'sh_k, sw_k' in doc and 'h_k, w_k' in doc      # the descriptor
    assert 'segf_slide_grid(Hs_k, Ws_k, ch_k, cw_k, sh_k, sw_k)' in doc and 'image-major, then window order' in doc
    assert 'Ws_k-1-x0, Ws_k-1-x1' in doc and 'same weights' in doc                # the flip rule
    assert 'ascending (i, j) order' in doc and 'true IEEE fp32 division' in doc    # the window mean
    assert 'added in set order' in doc and 'same bits' in doc                       # the summation order
    assert 'n > SEGF_MSF_MAX_MAPS' in doc and 'by-value kernel argument' in doc and 'can be captured' in doc
    assert 'NOT divided by n' in doc and 'lowest class index' in doc
    res, args = hip._DECLS['segf_msf_slide_argmax_confmat']
    assert res is C.c_int and len(args) == 19 and args[4] == C.POINTER(C.c_void_p)
    assert len(hip._DECLS['segf_msf_slide_supported'][1]) == 7
    assert callable(hip.msf_slide_argmax_confmat)


def _call(B=2, Cc=19, n=2, geom=None, ldl=None, H=24, W=40, prob=False, ldp=0, dt=0, ptrs=None, arrays=True):
    """Both entries with placeholder device pointers (never dereferenced: every case here is refused before a launch)."""
    lib = _lib()
    m = max(n, 1)
    geom = geom if geom is not None else [GOOD_GEOM[k % 2] for k in range(m)]
    flat = [v for g in geom for v in g]
    ldl = ldl if ldl is not None else [Cc] * m
    c_ptrs = (C.c_void_p * m)(*(ptrs if ptrs is not None else [0x1000] * m))
    c_geom = (C.c_int * len(flat))(*flat)
    c_ld = (C.c_int64 * len(ldl))(*ldl)
    c_fl = (C.c_int * m)(*[k & 1 for k in range(m)])
    sup = lib.segf_msf_slide_supported(dt, B, Cc, n, c_geom, H, W)
    rc = lib.segf_msf_slide_argmax_confmat(dt, B, Cc, n, c_ptrs if arrays else None, c_geom, c_ld, c_fl, H, W, None, 255, None, None, None,
                                           None, 0x2000 if prob else None, ldp, None)
    return sup, rc


def test_acceptable_shapes_are_supported():
    lib = _lib()
    g = (C.c_int * 16)(*(GOOD_GEOM[0] + GOOD_GEOM[1]))
    assert lib.segf_msf_slide_supported(0, 2, 19, 2, g, 24, 40) == 1
    assert lib.segf_msf_slide_supported(1, 65535, 192, 2, g, 1, 1) == 1                  # the limits are inclusive
    one = (C.c_int * 8)(4, 4, 4, 4, 4, 4, 6, 6)                                          # stride == crop == image, map larger than crop
    assert lib.segf_msf_slide_supported(1, 1, 1, 1, one, 9, 9) == 1
    assert lib.segf_msf_slide_supported(0, 2, 19, 2, None, 24, 40) == 0


def _bad(**kw):
    g = dict(zip(('Hs', 'Ws', 'ch', 'cw', 'sh', 'sw', 'h', 'w'), GOOD_GEOM[1]))
    g.update(kw)
    return [GOOD_GEOM[0], [g[k] for k in ('Hs', 'Ws', 'ch', 'cw', 'sh', 'sw', 'h', 'w')]]


@pytest.mark.parametrize('kw', [dict(n=0), dict(n=17), dict(Cc=0), dict(Cc=193), dict(B=0), dict(B=65536), dict(H=0), dict(W=0),
                                dict(geom=_bad(sh=0)), dict(geom=_bad(sw=0)), dict(geom=_bad(sh=13)), dict(geom=_bad(sw=17)),
                                dict(geom=_bad(ch=41)), dict(geom=_bad(cw=59)), dict(geom=_bad(ch=0, sh=0)), dict(geom=_bad(sh=-1)),
                                dict(geom=_bad(Hs=11)), dict(geom=_bad(Ws=15)), dict(geom=_bad(h=0)), dict(geom=_bad(w=0))],
                         ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()).replace(' ', ''))
def test_refused_by_both_entries(kw):
    sup, rc = _call(**kw)
    assert sup == 0 and rc == ERR_SHAPE


@pytest.mark.parametrize('kw', [dict(ldl=[19, 18]), dict(prob=True, ldp=18), dict(ptrs=[0x1000, None]), dict(arrays=False)],
                         ids=['ldl<C', 'ldp<C', 'logits[1]=NULL', 'logits=NULL'])
def test_refused_by_the_main_entry(kw):
    """Row strides and pointers are not part of segf_msf_slide_supported's signature: the main entry refuses them."""
    sup, rc = _call(**kw)
    assert sup == 1 and rc == ERR_SHAPE


def test_unknown_dtype():
    sup, rc = _call(dt=7)
    assert sup == 0 and rc == ERR_DTYPE


def test_dry_run_reaches_the_kernel_of_each_class_count():
    """The limits are inclusive: n = 16 and C = 192 are launched (dry run: the decision is recorded, nothing runs), and the class
    count picks the lane group (16 / 32 / 64 lanes per pixel) and the slots per lane."""
    from segmentation_factory_amd import hip
    lib = _lib()
    for Cc, want in ((2, '1, 16>'), (16, '1, 16>'), (19, '1, 32>'), (33, '1, 64>'), (64, '1, 64>'), (65, '2, 64>'), (150, '3, 64>'),
                     (192, '3, 64>')):
        for dt in (0, 1):
            n = 16
            flat = [v for k in range(n) for v in GOOD_GEOM[k % 2]]
            ptrs = (C.c_void_p * n)(*[0x1000] * n)
            c_geom = (C.c_int * len(flat))(*flat)
            c_ld = (C.c_int64 * n)(*[Cc + 3] * n)
            c_fl = (C.c_int * n)(*[k & 1 for k in range(n)])
            with hip.trace(dry_run=True) as t:
                rc = lib.segf_msf_slide_argmax_confmat(dt, 2, Cc, n, ptrs, c_geom, c_ld, c_fl, 24, 40, None, 255, None, None, None, None,
                                                       0x2000, Cc, None)
            assert rc == 0 and t.launches == 1, (Cc, rc, t.kernels)
            assert 'msf_slide_argmax_confmat_kernel' in t.kernels[0] and want in t.kernels[0].replace('T = ', ''), t.kernels


def test_cli_mode():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_gpu_cli_msf_slide', os.path.join(ROOT, 'train_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser(parents=[mod.get_args_parser()])
    args = parser.parse_args(['--eval-mode', 'slide-msf', '--eval-crop', '1024', '--eval-stride', '768', '--eval-scales', '0.5', '1.0',
                              '--eval-flip', '--eval-window-batch', '4'])
    assert args.eval_mode == 'slide-msf' and args.eval_crop == [1024] and args.eval_stride == [768]
    assert args.eval_scales == [0.5, 1.0] and args.eval_flip is True and args.eval_window_batch == 4
    assert parser.parse_args([]).eval_mode == 'whole'
    text = parser.format_help()
    assert text.count('slide-msf') >= 5                  # the mode itself and the flags that say they are read by it


class _Stub:
    """A model that must never run."""

    def eval(self):
        return self

    def __call__(self, x):
        raise AssertionError('the model was run')


def _args(**kw):
    return types.SimpleNamespace(nb_classes=7, ignore_label=255, **kw)


def test_evaluate_slide_msf_on_an_empty_loader():
    """eval_mode == 'slide-msf' reaches evaluate_msf_slide with the arguments of both parents: no batch, empty matrices, no forward."""
    from segmentation_factory_amd import engine
    for kw in (dict(eval_crop=[64]), dict(eval_crop=[64, 96], eval_stride=[48], eval_scales=[0.5, 1.0], eval_flip=True, eval_window_batch=4),
               dict(image_size=64, eval_flip=True)):
        confmat, metric = engine.evaluate(_args(eval_mode='slide-msf', **kw), _Stub(), [], 'cpu', 10)
        assert float(metric.hist.sum()) == 0.0 and tuple(metric.hist.shape) == (7, 7)
    confmat, metric = engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10)       # the defaults: six scales, mirrored, crop 512
    assert float(metric.hist.sum()) == 0.0
    with pytest.raises(ValueError, match='eval_crop'):
        engine.evaluate(_args(eval_mode='slide-msf'), _Stub(), [], 'cpu', 10)


def test_evaluate_passes_the_arguments_on(monkeypatch):
    from segmentation_factory_amd import engine
    seen = {}
    monkeypatch.setattr(engine, 'evaluate_msf_slide', lambda *a, **k: seen.update(k) or 'result')
    a = _args(eval_mode='slide-msf', eval_crop=[64, 96], eval_stride=[48], eval_scales=[0.5, 1.0], eval_flip=True, eval_window_batch=4)
    assert engine.evaluate(a, _Stub(), [], 'cpu', 10) == 'result'
    assert seen == dict(scales=(0.5, 1.0), flip=True, crop=[64, 96], stride=[48], window_batch=4)


def test_more_than_16_sets_raise():
    from segmentation_factory_amd import engine
    with pytest.raises(ValueError, match='16'):
        engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10, scales=tuple(0.5 + 0.1 * k for k in range(9)), flip=True)
    with pytest.raises(ValueError, match='16'):
        engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10, scales=tuple(0.5 + 0.1 * k for k in range(17)), flip=False)
    with pytest.raises(ValueError):
        engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10, scales=(), flip=True)
    with pytest.raises(ValueError, match='window_batch'):
        engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10, window_batch=0)
    engine.evaluate_msf_slide(_args(), _Stub(), [], 'cpu', 10, scales=tuple(0.5 + 0.1 * k for k in range(8)), flip=True)      # 16: accepted


def test_plain_slide_still_refuses_scales_and_flip():
    from segmentation_factory_amd import engine
    for kw in (dict(eval_scales=[0.5, 1.0]), dict(eval_flip=True)):
        with pytest.raises(ValueError, match='several scales or mirrored are not built') as e:
            engine.evaluate(_args(eval_mode='slide', eval_crop=[64], **kw), _Stub(), [], 'cpu', 10)
        assert 'slide-msf' in str(e.value)                 # the pointer to the mode that has them


def test_semseg_predict_refuses_msf_slide_with_slide():
    from segmentation_factory_amd.inference import SemSeg
    ss = SemSeg.__new__(SemSeg)                            # the refusal comes before anything of the object is touched
    with pytest.raises(ValueError, match='msf_slide together with slide'):
        ss.predict(None, slide=(64, 48), msf_slide=(64, 48))
