"""Mix-FFN backward with fc2's data gradient formed inside pass A of the depthwise backward (segf_dwconv3x3_gelu_bwd_fc2,
dwconv3x3_walk_fc2_kernel): bit-equality with the two calls it replaces, at the kernel, at the autograd Function and in the choice the
default policy makes for the recorded batch-4 step."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, C_hidden, C_in), SEGFAC_DW_WALK_ROWS or None, image whose dys rows are all zero (DropPath) or None
CASES = [
    ((2, 5, 16, 128, 32), None, None),        # one 16-pixel run, a segment shorter than the walk's rotation, the seam between two images
    ((2, 9, 22, 128, 32), None, None),        # W ragged against both 16 and 4
    ((2, 9, 22, 128, 32), '3', None),         # ... with segment seams inside the map
    ((3, 1, 16, 128, 32), None, None),        # H = 1
    ((1, 70, 36, 256, 64), None, None),       # two K steps, four channel slabs, two default segments
    ((2, 9, 22, 128, 32), None, 1),           # a dropped sample
]


def _inputs(shape, zero_image):
    B, H, W, Cc, Cin = shape
    g = torch.Generator().manual_seed(11)
    M = B * H * W
    f = torch.randn(M, Cc, generator=g).to(torch.bfloat16).cuda()
    dys = torch.randn(M, Cin, generator=g).to(torch.bfloat16)
    if zero_image is not None:
        dys[zero_image * H * W:(zero_image + 1) * H * W] = 0
    dys = dys.cuda()
    w2 = (torch.randn(Cin, Cc, generator=g) * 0.2).to(torch.bfloat16).cuda()
    w9 = (torch.randn(Cc, 9, generator=g) * 0.3).cuda()
    b = torch.randn(Cc, generator=g).cuda()
    return f, dys, w2, w9, b


def _parent(hip, f, w9, b, dys, w2, shape):
    """(du, dx, dw, db) of the two calls the fused entry point replaces, in the walk form (the one-launch form of small maps leaves no du)."""
    B, H, W, Cc, Cin = shape
    dg = hip.gemm(1, dys, w2, B * H * W, Cc, Cin)
    du, dx = torch.empty_like(f), torch.empty_like(f)
    dw = torch.empty((Cc, 9), dtype=torch.float32, device=f.device)
    db = torch.empty(Cc, dtype=torch.float32, device=f.device)
    ws = torch.empty(int(hip.lib().segf_dwconv3x3_bwd_ws(B, H, W, Cc)), dtype=torch.float32, device=f.device)
    rc = hip.lib().segf_dwconv3x3_gelu_bwd(hip.BF16, B, H, W, Cc, f.data_ptr(), w9.data_ptr(), b.data_ptr(), 1, dg.data_ptr(), du.data_ptr(),
                                           dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    # the wrapper's own result (what the step uses) has these bits too
    dx_w, dw_w, db_w = hip.dwconv3x3_gelu_bwd(f, w9, b, dg, B, H, W, Cc, True)
    assert torch.equal(dx_w, dx) and torch.equal(dw_w, dw) and torch.equal(db_w, db)
    return du, dx, dw, db


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[0])) + (f'-rows{c[1]}' if c[1] else '') + ('-drop' if c[2] is not None else ''))
def test_fused_entry_point_equals_gemm_then_depthwise_backward(case, monkeypatch):
    """du, dx, dw, db of segf_dwconv3x3_gelu_bwd_fc2 against hip.gemm(1, dys, W2, M, C_hidden, C_in) + hip.dwconv3x3_gelu_bwd, with the
    direct and with the deferred finalize: torch.equal on all four."""
    from segmentation_factory_amd import hip
    shape, rows, zero_image = case
    B, H, W, Cc, Cin = shape
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '2')
    monkeypatch.setenv('SEGFAC_DW_NO_SMALL', '1')            # both sides in the three-pass walk form: du exists, same partial-sum layout
    if rows:
        monkeypatch.setenv('SEGFAC_DW_WALK_ROWS', rows)
    assert hip.dwconv3x3_gelu_bwd_fc2_supported(torch.bfloat16, B, H, W, Cc, Cin)
    f, dys, w2, w9, b = _inputs(shape, zero_image)
    du0, dx0, dw0, db0 = _parent(hip, f, w9, b, dys, w2, shape)
    with hip.trace() as t:
        dx1, dw1, db1, du1 = hip.dwconv3x3_gelu_bwd_fc2(f, w9, b, dys, w2, B, H, W, Cc, Cin, return_du=True)
    assert any('dwconv3x3_walk_fc2_kernel' in k for k in t.kernels), t.kernels
    flat = torch.zeros(10 * Cc, dtype=torch.float32, device='cuda')
    dx2, item, du2 = hip.dwconv3x3_gelu_bwd_fc2(f, w9, b, dys, w2, B, H, W, Cc, Cin, dw_out=flat[:9 * Cc].view(Cc, 9), db_out=flat[9 * Cc:],
                                                defer=True, return_du=True)
    hip.colreduce_finalize_grouped([item])
    torch.cuda.synchronize()
    for name, got, want in (('du', du1, du0), ('dx', dx1, dx0), ('dw', dw1, dw0), ('db', db1, db0), ('du deferred', du2, du0),
                            ('dx deferred', dx2, dx0), ('dw deferred', flat[:9 * Cc].view(Cc, 9), dw0), ('db deferred', flat[9 * Cc:], db0)):
        d = (got.float() - want.float()).abs().max().item()
        print(f'{shape} rows={rows} drop={zero_image} {name}: max |diff| {d:.3e}, unequal elements {(got != want).sum().item()}')
    assert torch.equal(du1, du0) and torch.equal(dx1, dx0) and torch.equal(dw1, dw0) and torch.equal(db1, db0)
    assert torch.equal(du2, du0) and torch.equal(dx2, dx0)
    assert torch.equal(flat[:9 * Cc].view(Cc, 9), dw0) and torch.equal(flat[9 * Cc:], db0)
    if zero_image is not None:
        assert not du1[zero_image * H * W:(zero_image + 1) * H * W].any()


def test_mit_block_is_bit_equal_with_and_without_the_fused_backward(monkeypatch):
    """One MiT Block (dim 32, 16 x 24 map, batch 2, DropPath scales given, one sample dropped in the FFN branch) under
    SEGFAC_FFN_BWD_FUSED=2 and =0: output, input gradient and every parameter gradient bit-equal.  (SEGFAC_DW_NO_SMALL=1 in both runs:
    the fused form exists where the three-pass walk form is in use, which a 16 x 24 map takes only with the one-launch form off.)"""
    from segmentation_factory_amd import dispatch
    from segmentation_factory_amd.backbones import Block
    torch.manual_seed(7)
    B, H, W, dim = 2, 16, 24, 32
    blk = Block(dim, 1, sr_ratio=1, dpr=0.1).cuda()
    x0 = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    dy = torch.randn(B * H * W, dim).cuda().to(torch.bfloat16)
    s1 = torch.tensor([1.0 / 0.9, 1.0 / 0.9], device='cuda')
    s2 = torch.tensor([1.0 / 0.9, 0.0], device='cuda')
    monkeypatch.setenv('SEGFAC_DW_NO_SMALL', '1')
    outs, fused_calls = [], []
    for pol in ('2', '0'):
        monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', pol)
        x = x0.clone().requires_grad_()
        for p in blk.parameters():
            p.grad = None
        with dispatch.record() as calls:
            y = blk.tokens(x, B, H, W, (s1, s2))
            y.backward(dy)
        torch.cuda.synchronize()
        fused_calls.append(sum(c['fn'] == 'segf_dwconv3x3_gelu_bwd_fc2' for c in calls))
        outs.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    assert fused_calls == [1, 0], fused_calls
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2]) and len(outs[0][2]) >= 16
    for k, gnew in outs[0][2].items():
        assert torch.equal(gnew, outs[1][2][k]), k


def test_default_policy_leaves_the_batch4_step_on_the_two_launch_path():
    """tests/golden/dispatch_table.json records cfg2 at batch 4 with the parent's calls: under the default policy the live step makes no
    call of the new entry point (stage 1 at 65536 and stage 2 at 16384 token rows are below the size rule)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_dispatch_table
        entries = make_dispatch_table.record_case('cfg2', 4, False)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    names = {e['fn'] for e in entries}
    assert 'segf_dwconv3x3_gelu_bwd' in names and 'segf_dwconv3x3_gelu_bwd_fc2' not in names
