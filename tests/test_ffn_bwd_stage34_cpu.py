"""Host side of the fused Mix-FFN backward at the MiT stage-3 / stage-4 widths (C_in = 160, 256; segf_dwconv3x3_gelu_bwd_fc2_lds_supported and
the LDS form of dwconv3x3_walk_fc2_kernel): the shape / size / policy rule, the workspace and the kernels a call launches, without a GPU."""
import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
S3 = lambda B: (B, 32, 32, 640, 160)          # noqa: E731   cfg2 (SegFormer-B0, 512^2): stage 3 ...
S4 = lambda B: (B, 16, 16, 1024, 256)         # noqa: E731   ... and stage 4


def test_supported_follows_shape_size_and_policy(monkeypatch):
    from segmentation_factory_amd import hip
    sup, old = hip.dwconv3x3_gelu_bwd_fc2_lds_supported, hip.dwconv3x3_gelu_bwd_fc2_supported
    assert hip.policy('ffn_bwd_fused') == 1
    for s in (S3(4), S4(4)):
        assert not sup(BF16, *s), s                                # the recorded batch-4 step (4096 and 1024 token rows) stays as it is
    # C_in = 160 from 16384 rows on (where the A/B run still has it at 0.78 of the pair), below that the pair
    assert sup(BF16, *S3(256)) and sup(BF16, *S3(128)) and sup(BF16, *S3(16)) and not sup(BF16, 15, 32, 32, 640, 160)
    assert not sup(F32, *S3(256))
    for s in (S3(256), S4(256)):
        assert not old(BF16, *s), s                                # the register form's answer has not moved
    assert not sup(BF16, 256, 128, 128, 128, 32) and not sup(BF16, 256, 32, 32, 600, 160)      # other widths; C_hidden % 64
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '0')
    assert not sup(BF16, *S3(256)) and not sup(BF16, *S4(256))
    monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', '2')
    for s in (S3(256), S4(256), S3(16)):
        assert sup(BF16, *s), s
    assert not sup(BF16, *S3(4)) and not sup(BF16, *S4(4))         # maps the one-launch backward takes: the walk form is not in use
    monkeypatch.setenv('SEGFAC_DW_NO_SMALL', '1')
    assert sup(BF16, *S3(4)) and sup(BF16, *S4(4)) and sup(BF16, 3, 5, 7, 1024, 256)
    monkeypatch.setenv('SEGFAC_DW_NO_WALK', '1')
    assert not sup(BF16, *S3(256))


def test_stage4_row_bound_under_the_default_policy():
    """Stage 4 has a quarter of stage 3's token rows, so its bound under policy value 1 is its own (profiles/ffn_bwd_stage34_ab.jsonl); either
    way above the 1024 rows of the batch-4 step."""
    from segmentation_factory_amd import hip
    sup = hip.dwconv3x3_gelu_bwd_fc2_lds_supported
    assert sup(BF16, *S4(256)) == sup(BF16, *S4(128))
    assert not sup(BF16, *S4(16)) and not sup(BF16, *S4(4))


@pytest.mark.parametrize('shape,ks', [(S3(256), 5), (S4(256), 8), (S3(128), 5)])
def test_dry_run_names_the_lds_kernel_and_the_two_unchanged_ones(shape, ks):
    from segmentation_factory_amd import dispatch, hip
    B, H, W, Cc, Cin = shape
    lib = hip.lib()
    p = dispatch._PLACEHOLDER
    assert lib.segf_dwconv3x3_bwd_ws(B, H, W, Cc) >= lib.segf_dwconv3x3_bwd_blocks(hip.BF16, B, H, W, Cc) * 10 * Cc + 10 * Cc
    for dw in (None, p + 0x800):
        with hip.trace(dry_run=True) as t:
            rc = lib.segf_dwconv3x3_gelu_bwd_fc2(hip.BF16, B, H, W, Cc, Cin, p, p + 0x100, p + 0x200, p + 0x300, Cin, p + 0x400, p + 0x500,
                                                 p + 0x600, dw, None if dw is None else p + 0x900, p + 0x700, None)
        assert rc == 0
        assert len(t.kernels) == (3 if dw is None else 5), t.kernels
        assert t.kernels[0].startswith(f'dwconv3x3_walk_fc2_kernel<{ks}>'), t.kernels
        assert t.kernels[1].startswith('dwconv3x3_wgrad_walk_kernel<T>'), t.kernels
        assert t.kernels[2].startswith('dwconv3x3_walk_kernel<T, MODE>') and 'MODE = 1' in t.kernels[2], t.kernels
    assert lib.segf_dwconv3x3_gelu_bwd_fc2(hip.F32, B, H, W, Cc, Cin, p, p, p, p, Cin, p, p, p, None, None, p, None) != 0
    assert lib.segf_dwconv3x3_gelu_bwd_fc2(hip.BF16, B, H, W, Cc, 96, p, p, p, p, 96, p, p, p, None, None, p, None) != 0
