"""Host side of `LayerNorm -> thin Linear` in one pass (segf_layernorm_linear_fwd, ln_linear_fwd_kernel) and of the general fused backward
(segf_layernorm_linear_bwd_ex): the shape / size / policy rules, the block-count and workspace functions against hand arithmetic, and the
kernels a call launches -- without a GPU."""
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
# cfg2 (SegFormer-B0, 512^2): stages 1 and 2 at batch 4 and 256, (rows, C); each with the q Linear (N = C) and fc1 (N = 4 C)
B4 = [(4 * 128 * 128, 32), (4 * 64 * 64, 64)]
B256 = [(256 * 128 * 128, 32), (256 * 64 * 64, 64)]


def _both(shapes):
    return [(rows, C, n * C) for rows, C in shapes for n in (1, 4)]


def test_forward_supported_follows_dtype_shape_size_and_policy(monkeypatch):
    from segmentation_factory_amd import hip
    sup = hip.layernorm_linear_fwd_supported
    assert hip.policy('ln_linear_fwd_fused') == 1
    for s in _both(B4):
        assert not sup(BF16, *s), s                                # the recorded batch-4 step stays on its two launches
    for s in _both(B256):
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert sup(BF16, 131072, 32, 32) and not sup(BF16, 131071, 32, 32)
    assert sup(BF16, 131072, 64, 256) and not sup(BF16, 131071, 64, 256)
    assert not sup(BF16, 256 * 32 * 32, 160, 160) and not sup(BF16, 256 * 32 * 32, 160, 640) and not sup(BF16, 256 * 16 * 16, 256, 1024)   # stages 3 / 4
    assert not sup(BF16, 1 << 22, 32, 64) and not sup(BF16, 1 << 22, 64, 128) and not sup(BF16, 1 << 22, 32, 256)      # N is neither C nor 4 C
    assert not sup(BF16, 1 << 31, 32, 32) and sup(BF16, (1 << 31) - 1, 32, 32)
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '0')
    for s in _both(B4 + B256):
        assert not sup(BF16, *s), s
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '2')
    for s in _both(B4 + B256) + [(37, 32, 32), (37, 32, 128), (64, 64, 64), (1, 64, 256)]:
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert not sup(BF16, 256 * 32 * 32, 160, 640) and not sup(BF16, 1 << 22, 32, 64)
    assert not sup(BF16, 0, 32, 128)


def test_general_backward_supported_obeys_the_backward_switch(monkeypatch):
    from segmentation_factory_amd import hip
    sup, old = hip.layernorm_linear_bwd_ex_supported, hip.layernorm_linear_bwd_supported
    for s in _both(B4):
        assert not sup(BF16, *s), s
    for s in _both(B256):
        assert sup(BF16, *s) and not sup(F32, *s), s
    assert not old(BF16, 1 << 22, 32, 32) and sup(BF16, 1 << 22, 32, 32)          # N = C: the general entry point only
    assert sup(BF16, 131072, 64, 64) and not sup(BF16, 131071, 64, 64)
    assert not sup(BF16, 1 << 22, 32, 64) and not sup(BF16, 1 << 22, 160, 160)
    monkeypatch.setenv('SEGFAC_LN_LINEAR_FWD_FUSED', '2')                         # (the forward switch does not move the backward rule)
    assert not sup(BF16, 1024, 32, 32)
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '2')
    assert sup(BF16, 1024, 32, 32) and sup(BF16, 37, 64, 64) and sup(BF16, 37, 64, 256)
    monkeypatch.setenv('SEGFAC_LN_LINEAR_BWD_FUSED', '0')
    for s in _both(B256):
        assert not sup(BF16, *s), s


def test_block_count_and_workspace_against_hand_arithmetic():
    from segmentation_factory_amd import hip
    lib = hip.lib()
    # forward: a workgroup's four waves take at least four 16-token groups each; at most 2048 workgroups
    for rows, want in ((1, 1), (16, 1), (256, 1), (257, 2), (1620, 7), (131072, 512), (524288, 2048), (256 * 128 * 128, 2048), (0, 0)):
        assert lib.segf_layernorm_linear_fwd_blocks(rows) == want, rows
        if rows:
            assert want == min(-(-(-(-rows // 16)) // 16), 2048)
    # backward: tiles of 64 rows, at most 512 workgroups; per workgroup the partials of dW [N][C], db [N], dgamma | dbeta [2][C]
    for rows, nblk in ((37, 1), (64, 1), (65, 2), (1620, 26), (1 << 22, 512)):
        assert lib.segf_layernorm_linear_bwd_blocks(rows) == nblk
        for C in (32, 64):
            assert lib.segf_layernorm_linear_bwd_ws(rows, C, C) == nblk * (C * C + C + 2 * C)
            assert lib.segf_layernorm_linear_bwd_ws(rows, C, 4 * C) == nblk * (4 * C * C + 4 * C + 2 * C)
    assert lib.segf_layernorm_linear_bwd_ws(1620, 32, 32) == 26 * 1120 and lib.segf_layernorm_linear_bwd_ws(1620, 64, 64) == 26 * 4288


FWD_KERNELS = {(32, 32): (1, 2, 1), (32, 128): (1, 8, 1), (64, 64): (2, 4, 1), (64, 256): (2, 8, 2)}


@pytest.mark.parametrize('C,N', sorted(FWD_KERNELS))
def test_forward_dry_run_names_the_kernel(C, N):
    """One launch; its (KS, NT) are those of the gemm_skinny_kernel<0, KS, NT> that segf_gemm takes for the product at streaming sizes (the
    C = 64 -> 256 product's two column chunks are looped inside the one launch)."""
    from segmentation_factory_amd import dispatch, hip
    lib, p = hip.lib(), dispatch._PLACEHOLDER
    rows = 256 * 64 * 64
    ks, nt, nch = FWD_KERNELS[(C, N)]
    with hip.trace(dry_run=True) as t:           # the product it replaces: segf_gemm, layout 0, bf16, bias, dense rows
        assert lib.segf_gemm(hip.BF16, 0, rows, N, C, p, C, p + 0x100, C, p + 0x200, hip.BF16, N, p + 0x300, None, 0, None, 1, 1, None, None) == 0
    assert len(t.kernels) == 1 and t.kernels[0].startswith(f'gemm_skinny_kernel<LAYOUT, {ks}, {nt}>'), t.kernels
    for y, y2 in ((None, None), (p + 0x900, None), (None, p + 0xa00), (p + 0x900, p + 0xa00)):
        with hip.trace(dry_run=True) as t:
            rc = lib.segf_layernorm_linear_fwd(hip.BF16, rows, C, N, p, p + 0x100, p + 0x200, 1e-5, p + 0x300, p + 0x400, p + 0x500, p + 0x600,
                                               p + 0x700, y, y2, 6, 2, None)
        assert rc == 0
        want = f'ln_linear_fwd_kernel<{ks}, {nt}, {nch}, {"true" if y else "false"}, {"true" if y2 else "false"}>'
        assert len(t.kernels) == 1 and t.kernels[0].startswith(want), (t.kernels, want)


def test_forward_entry_point_is_replayable_and_refuses_what_it_has_no_kernel_for():
    from segmentation_factory_amd import dispatch, hip
    lib, p = hip.lib(), dispatch._PLACEHOLDER
    for name in ('segf_layernorm_linear_fwd', 'segf_layernorm_linear_fwd_supported', 'segf_layernorm_linear_bwd_ex', 'segf_layernorm_linear_bwd_ex_supported'):
        assert dispatch._replayable(name), name

    def call(dt, rows, C, N, y2=None, lw=5, ls=3, x=p, bias=p):
        with hip.trace(dry_run=True):
            return lib.segf_layernorm_linear_fwd(dt, rows, C, N, x, p, p, 1e-5, p, bias, p, p, p, None, y2, lw, ls, None)
    assert call(hip.BF16, 4096, 32, 32) == 0 and call(hip.BF16, 4096, 64, 256) == 0
    assert call(hip.F32, 4096, 32, 32) != 0                        # fp32 storage: an error, not another path
    assert call(hip.BF16, 4096, 160, 160) != 0 and call(hip.BF16, 4096, 32, 64) != 0 and call(hip.BF16, 0, 32, 32) != 0
    assert call(hip.BF16, 4096, 32, 32, bias=None) != 0            # the product it restates always adds a bias
    assert call(hip.BF16, 4096, 32, 32, x=p + 8) != 0              # 16-byte rows
    assert call(hip.BF16, 2 * 16 * 32, 32, 32, y2=p) == 0          # a 16 x 32 map, sr 8
    assert call(hip.BF16, 2 * 16 * 32 + 32, 32, 32, y2=p) != 0     # ... rows that are no whole number of sr-row bands
    assert call(hip.BF16, 2 * 16 * 32, 32, 32, y2=p, lw=2, ls=3) != 0


@pytest.mark.parametrize('C,N,fan', [(32, 128, False), (64, 256, False), (32, 32, True), (64, 64, True), (32, 32, False), (64, 64, False)])
def test_general_backward_dry_run(C, N, fan):
    """y == NULL: the rebuilding form of the kernel, <KS, true, N / C, fan-in>; one launch deferred, three finalizes behind it immediate."""
    from segmentation_factory_amd import dispatch, hip
    lib, p = hip.lib(), dispatch._PLACEHOLDER
    rows = 2 * 16 * 32

    def call(y=None, beta=p + 0x40, dy2=(p + 0x80) if fan else None, lw=5, ls=3, now=False, n=N):
        outs = [p + 0x900, p + 0xa00, p + 0xb00, p + 0xb00 + 4 * C] if now else [None] * 4
        with hip.trace(dry_run=True) as t:
            rc = lib.segf_layernorm_linear_bwd_ex(hip.BF16, rows, C, n, p, p + 0x100, p + 0x200, y, beta, dy2, lw, ls, p + 0x400, p + 0x500,
                                                  p + 0x600, p + 0x700, p + 0x800, p + 0xc00, 512, p + 0xd00, None, *outs, p + 0xe00, None)
        return rc, t.kernels
    for now in (False, True):
        rc, ks = call(now=now)
        assert rc == 0 and len(ks) == (4 if now else 1), ks
        want = f'ln_linear_bwd_kernel<{C // 32}, true, {N // C}, {"true" if fan else "false"}>'
        assert ks[0].startswith(want), (ks, want)
        assert all(k.startswith('colreduce_finalize') for k in ks[1:]), ks
    assert call(beta=None)[0] != 0                                 # nothing to rebuild y from
    if N == 4 * C:
        rc, ks = call(y=p + 0x300)                                 # a stored y: the kernel of segf_layernorm_linear_bwd itself
        assert rc == 0 and ks[0].startswith(f'ln_linear_bwd_kernel<{C // 32}>'), ks
        assert call(dy2=p + 0x80)[0] != 0                          # the fan-in operand belongs to the N == C form
    else:
        assert call(y=p + 0x300)[0] != 0
        if fan:
            assert call(lw=-1)[0] == 0                             # the fan-in in token order
            assert call(lw=2, ls=3)[0] != 0                        # a map narrower than the patch
    assert call(n=2 * C)[0] != 0
