"""Host side of the fused Mix-FFN backward (segf_dwconv3x3_gelu_bwd_fc2): the size / shape / policy rule and the kernels a call launches,
without a GPU."""
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
B4 = [(4, 128, 128, 128, 32), (4, 64, 64, 256, 64)]              # cfg2 (SegFormer-B0, 512^2) at batch 4: stages 1 and 2
B256 = [(256, 128, 128, 128, 32), (256, 64, 64, 256, 64)]


def test_supported_follows_shape_size_and_policy(monkeypatch):
    from segmentation_factory_amd import hip
    sup = hip.dwconv3x3_gelu_bwd_fc2_supported
    assert hip.policy('ffn_bwd_fused') == 1
    for s in B4:
        assert not sup(BF16, *s), s                                # the recorded batch-4 step stays on its two launches
    for s in B256:
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert not sup(BF16, 256, 32, 32, 640, 160)                    # C_in = 160 (stage 3)
    assert not sup(BF16, 256, 128, 128, 96, 32)                    # C_hidden = 96
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '0')
    for s in B256:
        assert not sup(BF16, *s), s
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '2')
    for s in B4 + B256:
        assert sup(BF16, *s), s
        assert not sup(F32, *s), s
    assert not sup(BF16, 256, 32, 32, 640, 160) and not sup(BF16, 256, 128, 128, 96, 32)
    assert not sup(BF16, 2, 16, 24, 128, 32)                       # a map the one-launch backward takes: the walk form is not in use
    monkeypatch.setenv('SEGFAC_DW_NO_SMALL', '1')
    assert sup(BF16, 2, 16, 24, 128, 32)
    monkeypatch.setenv('SEGFAC_DW_NO_WALK', '1')
    assert not sup(BF16, *B256[0])


@pytest.mark.parametrize('shape,ks', [(B256[0], 1), (B256[1], 2)])
def test_dry_run_names_the_new_kernel_and_the_two_unchanged_ones(shape, ks):
    from segmentation_factory_amd import dispatch, hip
    B, H, W, Cc, Cin = shape
    p = dispatch._PLACEHOLDER
    for dw in (None, p + 0x800):
        with hip.trace(dry_run=True) as t:
            rc = hip.lib().segf_dwconv3x3_gelu_bwd_fc2(hip.BF16, B, H, W, Cc, Cin, p, p + 0x100, p + 0x200, p + 0x300, Cin, p + 0x400, p + 0x500,
                                                       p + 0x600, dw, None if dw is None else p + 0x900, p + 0x700, None)
        assert rc == 0
        assert len(t.kernels) == (3 if dw is None else 5), t.kernels
        assert t.kernels[0].startswith(f'dwconv3x3_walk_fc2_kernel<{ks}>'), t.kernels
        assert t.kernels[1].startswith('dwconv3x3_wgrad_walk_kernel<T>'), t.kernels
        assert t.kernels[2].startswith('dwconv3x3_walk_kernel<T, MODE>') and 'MODE = 1' in t.kernels[2], t.kernels
    # the entry point is a recordable / replayable call like every other
    assert dispatch._replayable('segf_dwconv3x3_gelu_bwd_fc2')
    assert hip.lib().segf_dwconv3x3_gelu_bwd_fc2(hip.F32, B, H, W, Cc, Cin, p, p, p, p, Cin, p, p, p, None, None, p, None) != 0
