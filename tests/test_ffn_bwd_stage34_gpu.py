"""Mix-FFN backward at the MiT stage-3 / stage-4 widths (C_in = 160 -> 640, 256 -> 1024): fc2's data gradient formed inside pass A of the
depthwise backward with the W2 fragments read from LDS (dwconv3x3_walk_fc2_kernel<5>, <8>).  Every output bit-equal to segf_gemm
(layout 1) + segf_dwconv3x3_gelu_bwd on random operands, and inside the float64 bars tests/test_dwconv_float64.py applies to the forms
that exist at stages 1 and 2 (tests/dwconv_refs.py: lattice operands, so the gradient rows that never exist in memory are exact integers with
one known rounding)."""
import pytest
import torch

import dwconv_refs as D

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32

# (B, H, W, C_hidden, C_in)
SHAPES = [
    (2, 16, 16, 1024, 256),       # one 16-pixel run per row
    (1, 32, 32, 640, 160),
    (1, 12, 20, 640, 160),        # ragged last run; the seam between segments comes from SEGFAC_DW_WALK_ROWS = 5 below
    (3, 5, 7, 1024, 256),         # map smaller than a run
]
ROWS = {(1, 12, 20, 640, 160): 5}
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _force(monkeypatch, shape):
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '2')
    monkeypatch.setenv('SEGFAC_DW_NO_SMALL', '1')            # both sides in the three-pass walk form: du exists, same partial-sum layout
    if shape in ROWS:
        monkeypatch.setenv('SEGFAC_DW_WALK_ROWS', str(ROWS[shape]))


def _two_launches(hip, f, w9, b, dys, w2, shape):
    B, H, W, Cc, Cin = shape
    dg = hip.gemm(1, dys, w2, B * H * W, Cc, Cin)
    du, dx = torch.empty_like(f), torch.empty_like(f)
    dw = torch.empty((Cc, 9), dtype=F32, device=f.device)
    db = torch.empty(Cc, dtype=F32, device=f.device)
    ws = torch.empty(int(hip.lib().segf_dwconv3x3_bwd_ws(B, H, W, Cc)), dtype=F32, device=f.device)
    rc = hip.lib().segf_dwconv3x3_gelu_bwd(hip.BF16, B, H, W, Cc, f.data_ptr(), w9.data_ptr(), b.data_ptr(), 1, dg.data_ptr(), du.data_ptr(),
                                           dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return du, dx, dw, db


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_lds_form_equals_gemm_then_depthwise_backward(shape, monkeypatch):
    from segmentation_factory_amd import hip
    B, H, W, Cc, Cin = shape
    _force(monkeypatch, shape)
    assert hip.dwconv3x3_gelu_bwd_fc2_lds_supported(BF, B, H, W, Cc, Cin)
    g = torch.Generator().manual_seed(17)
    M = B * H * W
    f = torch.randn(M, Cc, generator=g).to(BF).cuda()
    dys = torch.randn(M, Cin, generator=g).to(BF).cuda()
    w2 = (torch.randn(Cin, Cc, generator=g) * 0.2).to(BF).cuda()
    w9 = (torch.randn(Cc, 9, generator=g) * 0.3).cuda()
    b = torch.randn(Cc, generator=g).cuda()
    du0, dx0, dw0, db0 = _two_launches(hip, f, w9, b, dys, w2, shape)
    with hip.trace() as t:
        dx1, dw1, db1, du1 = hip.dwconv3x3_gelu_bwd_fc2(f, w9, b, dys, w2, B, H, W, Cc, Cin, return_du=True)
    assert any(f'dwconv3x3_walk_fc2_kernel<{Cin // 32}>' in k for k in t.kernels), t.kernels
    assert not any('gemm' in k for k in t.kernels), t.kernels
    flat = torch.zeros(10 * Cc, dtype=F32, device='cuda')
    dx2, item, du2 = hip.dwconv3x3_gelu_bwd_fc2(f, w9, b, dys, w2, B, H, W, Cc, Cin, dw_out=flat[:9 * Cc].view(Cc, 9), db_out=flat[9 * Cc:],
                                                defer=True, return_du=True)
    hip.colreduce_finalize_grouped([item])
    torch.cuda.synchronize()
    pairs = (('du', du1, du0), ('dx', dx1, dx0), ('dw', dw1, dw0), ('db', db1, db0), ('du deferred', du2, du0), ('dx deferred', dx2, dx0),
             ('dw deferred', flat[:9 * Cc].view(Cc, 9), dw0), ('db deferred', flat[9 * Cc:], db0))
    for name, got, want in pairs:
        print(f'{shape} {name}: unequal elements {(got != want).sum().item()} of {want.numel()}')
    for name, got, want in pairs:
        assert torch.equal(got, want), name
    assert du0.float().abs().max().item() > 0


def _dev(t, dtype=F32):
    return t.reshape(-1, t.shape[-1]).to(dtype).cuda().contiguous() if t.dim() > 1 else t.to(dtype).cuda().contiguous()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_lds_form_against_float64(shape, monkeypatch):
    from segmentation_factory_amd import hip
    B, H, W, Cc, Cin = shape
    rows = ROWS.get(shape, 0)
    _force(monkeypatch, shape)
    case = dict(id=f'fc2-{D._sid(shape)}{f"-rows{rows}" if rows else ""}', k=3, shape=(B, H, W, Cc), cls='fc2', gelu=True)
    i = D.fc2_inputs(shape, rows)
    Y = D.make_yard(case, i, BF)
    assert hip.lib().segf_dwconv3x3_bwd_blocks(hip.BF16, B, H, W, Cc) == D.wgrad_blocks('walk', BF, B, H, W, Cc, rows)
    args = (_dev(i['x'], BF), _dev(i['w']), _dev(i['b']), _dev(i['dys'], BF), _dev(i['w2'], BF), B, H, W, Cc, Cin)
    dx, dw, db, du = hip.dwconv3x3_gelu_bwd_fc2(*args, return_du=True)
    torch.cuda.synchronize()
    verdicts = D.judge(Y, dict(du=du.cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu()))
    for name, v in verdicts.items():
        print(f'RATIO dw3.fc2.lds {name} {case["id"]} bf16 {v.ratio:.4g}')
    bad = [v.message for v in verdicts.values() if not v.ok]
    assert not bad, '\n'.join(bad)
