"""Host side of the multi-scale + flip evaluation (no GPU): the C ABI entries are declared, documented and exported, refuse the
shapes the header says they refuse before any launch, engine.msf_sizes rounds as documented and train_gpu.py has the two flags."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE = -1


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
    for name in ('segf_msf_supported', 'segf_msf_argmax_confmat'):
        assert name in hip.exported_symbols()
        assert hasattr(lib, name)
    assert re.search(r'#define\s+SEGF_MSF_MAX_MAPS\s+16\b', header) and hip.MSF_MAX_MAPS == 16
    doc = header[header.index('multi-scale + flip'):header.index('int segf_msf_supported')]
    doc = ' '.join(re.sub(r'^\s*\*\s', ' ', doc, flags=re.M).split())              # one line, comment margins removed
    assert 'w_k-1-x0, w_k-1-x1' in doc and 'same weights' in doc                  # the flip rule
    assert 'added in map order' in doc and 'same bits' in doc                       # the summation order
    assert 'n > SEGF_MSF_MAX_MAPS' in doc and 'by-value kernel argument' in doc     # the limit and why it exists
    assert 'NOT divided by n' in doc and 'lowest class index' in doc
    # the binding derived from the header: host arrays of pointers / ints / int64
    res, args = hip._DECLS['segf_msf_argmax_confmat']
    assert res is C.c_int and len(args) == 19 and args[4] == C.POINTER(C.c_void_p)


def _call(B=2, Cc=19, n=2, hw=None, ldl=None, H=8, W=8, prob=False, ldp=0, dt=0):
    """The main entry with placeholder device pointers (never dereferenced: every case here is refused before a launch)."""
    lib = _lib()
    m = max(n, 1)
    hw = hw if hw is not None else [4, 4] * m
    ldl = ldl if ldl is not None else [Cc] * m
    ptrs = (C.c_void_p * m)(*[0x1000] * m)
    c_hw = (C.c_int * len(hw))(*hw)
    c_ld = (C.c_int64 * len(ldl))(*ldl)
    c_fl = (C.c_int * m)(*[0] * m)
    sup = lib.segf_msf_supported(dt, B, Cc, n, c_hw, H, W)
    rc = lib.segf_msf_argmax_confmat(dt, B, Cc, n, ptrs, c_hw, c_ld, c_fl, H, W, None, 255, None, None, None, None,
                                     0x2000 if prob else None, ldp, None)
    return sup, rc


def test_acceptable_shape_is_supported():
    lib = _lib()
    hw = (C.c_int * 4)(4, 4, 9, 3)
    assert lib.segf_msf_supported(0, 2, 19, 2, hw, 8, 8) == 1
    assert lib.segf_msf_supported(1, 1, 192, 2, hw, 1, 1) == 1
    assert lib.segf_msf_supported(7, 2, 19, 2, hw, 8, 8) == 0          # no such dtype


@pytest.mark.parametrize('kw', [dict(n=0), dict(n=17), dict(Cc=0), dict(Cc=193), dict(B=65536), dict(H=0), dict(W=0),
                                dict(hw=[4, 4, 0, 4]), dict(hw=[4, 4, 4, 0])],
                         ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_refused_by_both_entries(kw):
    sup, rc = _call(**kw)
    assert sup == 0 and rc == ERR_SHAPE


@pytest.mark.parametrize('kw', [dict(ldl=[19, 18]), dict(prob=True, ldp=18)], ids=['ldl<C', 'ldp<C'])
def test_refused_by_the_main_entry(kw):
    """Row strides are not part of segf_msf_supported's signature: the main entry refuses them."""
    sup, rc = _call(**kw)
    assert sup == 1 and rc == ERR_SHAPE


def test_dry_run_reaches_the_kernel_of_each_class_count():
    """The limits are inclusive: n = 16 and C = 192 are launched (dry run: the decision is recorded, nothing runs), and the class
    count picks the lane group (16 / 32 / 64 lanes per pixel) and the slots per lane."""
    from segmentation_factory_amd import hip
    lib = _lib()
    for Cc, want in ((2, '1, 16>'), (16, '1, 16>'), (19, '1, 32>'), (33, '1, 64>'), (64, '1, 64>'), (65, '2, 64>'), (150, '3, 64>'),
                     (192, '3, 64>')):
        n = 16
        ptrs = (C.c_void_p * n)(*[0x1000] * n)
        c_hw = (C.c_int * (2 * n))(*[4, 4] * n)
        c_ld = (C.c_int64 * n)(*[Cc] * n)
        c_fl = (C.c_int * n)(*[k & 1 for k in range(n)])
        with hip.trace(dry_run=True) as t:
            rc = lib.segf_msf_argmax_confmat(1, 2, Cc, n, ptrs, c_hw, c_ld, c_fl, 8, 8, None, 255, None, None, None, None, None, 0, None)
        assert rc == 0 and t.launches == 1, (Cc, rc, t.kernels)
        assert 'msf_argmax_confmat_kernel' in t.kernels[0] and want in t.kernels[0].replace('T = ', ''), t.kernels


def test_msf_sizes():
    from segmentation_factory_amd.engine import MSF_SCALES, msf_sizes
    assert MSF_SCALES == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    assert msf_sizes(512, 512, MSF_SCALES) == [(s, s) for s in (256, 384, 512, 640, 768, 896)]
    assert msf_sizes(64, 96, (0.5, 1.0, 1.5)) == [(32, 64), (64, 96), (96, 160)]


def test_cli_flags():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_gpu_cli_msf', os.path.join(ROOT, 'train_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser(parents=[mod.get_args_parser()])
    args = parser.parse_args(['--eval-scales', '0.5', '1.0', '--eval-flip'])
    assert args.eval_scales == [0.5, 1.0] and args.eval_flip is True
    args = parser.parse_args([])
    assert not args.eval_scales and args.eval_flip is False
