"""CAS-ViT (RCViT) backbones, the parts that need no GPU: the float64 restatement of the token-mixer kernels against the reference's own
AdditiveTokenMixer (tests/golden/casvit_mixer_cases.npz), the module surface (names, state_dict inventory, channels, initialisation)
and the C ABI of csrc/token_mixer.hip (declarations, workspace arithmetic, host-side refusals, dry-run dispatch)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import casvit_refs as R

# (B, H, W, C): the kernel shape list of tests/test_casvit_gpu.py
KERNEL_SHAPES = [
    (1, 3, 4, 48),            # fewer rows than a wave; C not a multiple of 64
    (2, 5, 7, 64),            # per-sample sums must not mix samples
    (3, 9, 13, 128),          # three samples, one workgroup each, a partly filled last row group
    (2, 33, 20, 256),         # several workgroups per sample: the fixed-order cross-workgroup sums run
    (1, 5, 7, 512),           # the widest in-scope C
]
SLICE_SHAPE = (2, 18, 26, 96)     # operands as columns C .. 2C of a [M, 3C] buffer
WIDE_SHAPE = (1, 3, 5, 1024)      # the kernels' own limit: two chunks per lane

TOKEN_MIXER_ENTRIES = ('segf_spatial_gate_supported', 'segf_spatial_gate_fwd_ws', 'segf_spatial_gate_fwd', 'segf_spatial_gate_bwd_ws',
                       'segf_spatial_gate_bwd', 'segf_channel_gate_mix_supported', 'segf_channel_gate_mix_fwd',
                       'segf_channel_gate_mix_bwd_ws', 'segf_channel_gate_mix_bwd', 'segf_gated_mul_supported', 'segf_gated_mul_fwd',
                       'segf_gated_mul_bwd')


# ---- the restated formulas are the reference's ---------------------------------------------------------------------------------------------
def test_restated_mixer_matches_the_reference_fixture(golden_dir):
    """casvit_refs.mixer (float64, the three kernel pairs written out forward and backward, BatchNorm with batch statistics) against the
    reference module's fp32 output and input gradient: 1e-5 of scale."""
    from tools.make_casvit_goldens import MIXER_CASES, mixer_io, mixer_state_dict
    g = np.load(os.path.join(golden_dir, 'casvit_mixer_cases.npz'))
    assert [tuple(c) for c in g['cases']] == [tuple(c) for c in MIXER_CASES] == [(2, 48, 5, 7), (3, 64, 9, 13)]
    for i, (B, C, H, W) in enumerate(MIXER_CASES):
        x, dy = mixer_io(B, C, H, W, i)
        y, dx = R.mixer(x, mixer_state_dict(C, i), dy)
        for what, got, ref in (('y', y, g[f'y{i}']), ('dx', dx, g[f'dx{i}'])):
            ref = torch.from_numpy(ref).double()
            err = (got - ref).abs().max().item() / ref.abs().max().item()
            print(f'  case {i} {what}: err / scale {err:.3e}')
            assert got.shape == ref.shape and err <= 1e-5, (i, what, err)


def test_restated_backward_formulas_are_the_derivatives():
    """The backward restatements against autograd's derivative of the forward restatements (float64, 1e-10)."""
    torch.manual_seed(5)
    B, HW, C = 2, 6, 16
    x, r, dy = (torch.randn(B * HW, C, dtype=torch.float64) for _ in range(3))
    w, dpool = torch.randn(C, dtype=torch.float64), torch.randn(B, C, dtype=torch.float64)
    xa, ra, wa = (t.clone().requires_grad_(True) for t in (x, r, w))
    y, s, pool = R.spatial_gate_fwd(xa, ra, wa, B)
    ((y * dy).sum() + (pool * dpool).sum()).backward()
    for got, ref in zip(R.spatial_gate_bwd(dy, dpool, x, r, s.detach(), w, B), (xa.grad, ra.grad, wa.grad)):
        assert torch.allclose(got, ref, rtol=1e-10, atol=1e-10)
    gq, gk = torch.rand(B, C, dtype=torch.float64), torch.rand(B, C, dtype=torch.float64)
    args = [t.clone().requires_grad_(True) for t in (x, r, gq, gk)]
    (R.channel_gate_mix_fwd(*args) * dy).sum().backward()
    for got, a in zip(R.channel_gate_mix_bwd(dy, x, r, gq, gk), args):
        assert torch.allclose(got, a.grad, rtol=1e-10, atol=1e-10)
    args = [t.clone().requires_grad_(True) for t in (x, r)]
    (R.gated_mul_fwd(*args) * dy).sum().backward()
    for got, a in zip(R.gated_mul_bwd(dy, x, r), args):
        assert torch.allclose(got, a.grad, rtol=1e-10, atol=1e-10)


# ---- module surface --------------------------------------------------------------------------------------------------------------------------
def test_rcvit_s_state_dict_is_the_reference_inventory(golden_dir):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_casvit_goldens import load_inventory
    for fixture in ('e2e_rcvit_s_128x160.npz', 'e2e_rcvit_s_72x104.npz'):
        g = np.load(os.path.join(golden_dir, fixture))
        inv = load_inventory(g)
        assert len(inv) == 791
        m = SegmentationModel('rcvit_s', num_classes=int(g['nc']), seg_head='SegFormerHead')
        mine = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert mine == inv                                              # keys, shapes and order
    keys = {k for k, _ in mine}
    for k in ('backbone.patch_embed.0.weight', 'backbone.patch_embed.4.running_var', 'backbone.network.0.0.local_perception.network.4.bias',
              'backbone.network.2.1.attn.qkv.weight', 'backbone.network.2.1.attn.oper_q.0.block.3.weight',
              'backbone.network.4.5.attn.oper_k.1.block.1.weight', 'backbone.network.6.2.attn.proj.bias', 'backbone.network.6.2.mlp.fc2.bias',
              'backbone.network.1.proj.weight', 'backbone.network.5.norm.num_batches_tracked', 'backbone.norm6.weight'):
        assert k in keys, k
    sd = m.state_dict()
    assert sd['backbone.network.2.1.attn.qkv.weight'].shape == (192, 64, 1, 1)            # conv weights keep their 4-D shapes
    assert sd['backbone.network.2.1.attn.oper_q.0.block.3.weight'].shape == (1, 64, 1, 1)
    assert 'backbone.network.2.1.attn.qkv.bias' not in keys


@pytest.mark.parametrize('name,dims', [('rcvit_s', [48, 64, 128, 256]), ('rcvit_m', [64, 96, 192, 384]), ('rcvit_t', [96, 128, 256, 512])])
def test_factories_build(name, dims):
    from segmentation_factory_amd import SegmentationModel
    m = SegmentationModel(name, num_classes=7, seg_head='SegFormerHead')
    assert m.backbone.channels == dims
    assert [len(m.backbone.network[i]) for i in (0, 2, 4, 6)] == [3, 3, 6, 3]
    assert m.decode_head.state_dict()['linear_pred.weight'].shape[1] == 768          # quirk Q1: no 'tiny' / 'small' in the name
    assert not [n for n, mod in m.named_modules() if getattr(mod, 'drop_prob', 0) > 0]
    # nothing stochastic in the backbone at all: no drop path, no dropout
    assert not any(hasattr(mod, 'drop_prob') or isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout2d)) for mod in m.backbone.modules())


def test_rcvit_xs_and_crossformerpp_stay_key_errors():
    from segmentation_factory_amd import SegmentationModel
    with pytest.raises(KeyError, match=r'56, 112 and 220.*channel rule'):
        SegmentationModel('rcvit_xs', num_classes=7, seg_head='SegFormerHead')
    with pytest.raises(KeyError):
        SegmentationModel('crossformerpp_base', num_classes=7, seg_head='SegFormerHead')


def test_init_is_torch_default():
    """casvit.py:242-246: cls_init_weights touches nn.Linear only, so every Conv2d keeps kaiming_uniform(a = sqrt 5) (|w| <= 1 / sqrt(fan_in),
    bias uniform in the same bound) and every BatchNorm 1 / 0 with fresh running statistics."""
    from segmentation_factory_amd import backbones
    torch.manual_seed(0)
    m = backbones.rcvit_s()
    assert not any(isinstance(mod, torch.nn.Linear) for mod in m.modules())
    n_conv = n_bn = 0
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            n_conv += 1
            bound = 1.0 / math.sqrt(mod.weight[0].numel())
            w = mod.weight.detach()
            assert float(w.abs().max()) <= bound
            if w.numel() >= 4096:
                assert abs(float(w.std()) - bound / math.sqrt(3)) < 0.05 * bound
            if mod.bias is not None:
                assert 0 < float(mod.bias.detach().abs().max()) <= bound
        elif isinstance(mod, torch.nn.BatchNorm2d):
            n_bn += 1
            assert torch.equal(mod.weight, torch.ones_like(mod.weight)) and torch.equal(mod.bias, torch.zeros_like(mod.bias))
            assert torch.equal(mod.running_var, torch.ones_like(mod.running_var)) and int(mod.num_batches_tracked) == 0
            assert mod.momentum == 0.1 and mod.eps == 1e-5
    # per block: 3 + 1 + 2 * 3 + 2 + 2 convolutions and 1 + 1 + 2 + 1 BatchNorms; stem 2 + 2; three embeddings; four output norms
    assert n_conv == 15 * 14 + 2 + 3 and n_bn == 15 * 5 + 2 + 3 + 4


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_token_mixer_entries():
    from segmentation_factory_amd import hip
    with open(hip.HEADER_PATH) as fh:
        text = fh.read()
    lib = hip.lib()
    for name in TOKEN_MIXER_ENTRIES:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in hip.exported_symbols() and hasattr(lib, name)


def _plan(B, HW, C):
    """(lanes per row, workgroups per sample) of csrc/token_mixer.hip:tm_geom"""
    L = 1
    while L < C // 8 and L < 64:
        L *= 2
    RL = 256 // L
    nblk = min(-(-HW // (RL * 16)), max(4096 // B, 1))
    rpb = -(-HW // nblk)
    return L, -(-HW // rpb)


def test_workspace_sizes_follow_the_launch_geometry():
    """*_ws (host arithmetic): one [C] slab per workgroup -- B * workgroups-per-sample of them, twice that for the two gate gradients."""
    from segmentation_factory_amd import hip
    lib = hip.lib()
    per_sample = {}
    for B, H, W, C in KERNEL_SHAPES + [SLICE_SHAPE, WIDE_SHAPE, (64, 128, 128, 48), (64, 16, 16, 512)]:
        L, nblk = _plan(B, H * W, C)
        per_sample[(B, H, W, C)] = nblk
        assert lib.segf_spatial_gate_fwd_ws(B, H * W, C) == B * nblk * C
        assert lib.segf_spatial_gate_bwd_ws(B, H * W, C) == B * nblk * C
        assert lib.segf_channel_gate_mix_bwd_ws(B, H * W, C) == 2 * B * nblk * C
    assert per_sample[(2, 33, 20, 256)] == 6 and per_sample[(3, 9, 13, 128)] == 1 and per_sample[(64, 128, 128, 48)] == 32
    assert lib.segf_spatial_gate_fwd_ws(2, 35, 220) == 0 and lib.segf_channel_gate_mix_bwd_ws(2, 35, 220) == 0


def test_supported_queries_state_the_shape_rules():
    from segmentation_factory_amd import hip
    lib = hip.lib()
    for dt in (hip.F32, hip.BF16):
        for q in (lib.segf_spatial_gate_supported, lib.segf_channel_gate_mix_supported):
            for C in (48, 64, 96, 128, 192, 256, 384, 512, 1024):
                assert q(dt, 2, 35, C, C) == 1 and q(dt, 2, 35, C, 3 * C) == 1
            assert q(dt, 2, 35, 220, 220) == 0 and q(dt, 2, 35, 220, 224) == 0           # C % 8
            assert q(dt, 2, 35, 1032, 1032) == 0 and q(dt, 2, 35, 0, 8) == 0              # C <= 1024, C > 0
            assert q(dt, 2, 35, 64, 66) == 0 and q(dt, 2, 35, 64, 56) == 0                # misaligned rows; ld < C
            assert q(dt, 1 << 14, 1 << 15, 64, 64) == 0 and q(dt, 1 << 14, (1 << 15) - 1, 64, 64) == 1       # B HW < 2^31 / 4
            assert q(dt, 0, 35, 64, 64) == 0 and q(dt, 2, 0, 64, 64) == 0
        assert lib.segf_gated_mul_supported(dt, 70, 64, 192) == 1 and lib.segf_gated_mul_supported(dt, 70, 220, 220) == 0
        assert lib.segf_gated_mul_supported(dt, 70, 64, 66) == 0 and lib.segf_gated_mul_supported(dt, 1 << 29, 64, 64) == 0
    assert lib.segf_spatial_gate_supported(hip.F32, 2, 35, 64, 68) == 1 and lib.segf_spatial_gate_supported(hip.BF16, 2, 35, 64, 68) == 0
    assert lib.segf_spatial_gate_supported(7, 2, 35, 64, 64) == 0                         # no such dtype


def _dry_calls(lib, dt, B, HW, C, ld):
    """Every launching entry point once, as a dry run (placeholder pointers, nothing is launched); -> return codes"""
    p = 1 << 20          # any 16-byte aligned non-null address
    M = B * HW
    return [lib.segf_spatial_gate_fwd(dt, B, HW, C, p, ld, p, p, p, p, ld, p, p, None),
            lib.segf_spatial_gate_bwd(dt, B, HW, C, p, ld, p, p, ld, p, p, p, p, ld, p, p, p, None),
            lib.segf_channel_gate_mix_fwd(dt, B, HW, C, p, ld, p, ld, p, p, p, ld, None),
            lib.segf_channel_gate_mix_bwd(dt, B, HW, C, p, ld, p, ld, p, ld, p, p, p, ld, p, ld, p, p, p, None),
            lib.segf_gated_mul_fwd(dt, M, C, p, ld, p, ld, p, ld, None),
            lib.segf_gated_mul_bwd(dt, M, C, p, ld, p, ld, p, ld, p, ld, p, ld, None)]


def test_dry_run_dispatch_and_host_refusals():
    """The kernels each entry point launches (a dry-run trace: no GPU), one chunk per lane up to C = 512 and two above; a bad shape, a
    misaligned leading dimension or a misaligned pointer returns SEGF_ERR_SHAPE and a missing workspace SEGF_ERR_WORKSPACE with NO launch."""
    from segmentation_factory_amd import hip
    lib = hip.lib()
    for dt in (hip.F32, hip.BF16):
        for (B, H, W, C), ni in ((KERNEL_SHAPES[3], 1), (KERNEL_SHAPES[4], 1), (WIDE_SHAPE, 2)):
            with hip.trace(dry_run=True) as t:
                rcs = _dry_calls(lib, dt, B, H * W, C, 3 * C)
            assert rcs == [0] * 6, rcs
            names = [re.sub(r'\s+', '', k) for k in t.kernels]
            want = ['spatial_gate_fwd_kernel', 'colreduce_finalize_kernel', 'spatial_gate_bwd_kernel', 'colreduce_finalize_kernel',
                    'channel_gate_mix_fwd_kernel', 'channel_gate_mix_bwd_kernel', 'colreduce_finalize_kernel', 'colreduce_finalize_kernel',
                    'gated_mul_fwd_kernel', 'gated_mul_bwd_kernel']
            assert len(names) == len(want) and all(w in n for w, n in zip(want, names)), t.kernels
            assert all(f'<T,{ni}>' in n for n in names if 'colreduce' not in n), t.kernels
        for B, HW, C, ld in ((2, 35, 220, 220), (2, 35, 64, 66), (2, 35, 2048, 2048), (2, 0, 64, 64)):
            with hip.trace(dry_run=True) as t:
                rcs = _dry_calls(lib, dt, B, HW, C, ld)
            assert rcs == [hip.ERR_SHAPE] * 6 and t.kernels == [], (B, HW, C, ld, rcs, t.kernels)
        with hip.trace(dry_run=True) as t:
            p = 1 << 20
            assert lib.segf_gated_mul_fwd(dt, 70, 64, p + 8, 64, p, 64, p, 64, None) == hip.ERR_SHAPE          # pointer not 16-byte aligned
            assert lib.segf_spatial_gate_fwd(dt, 2, 35, 64, p, 64, p, p, p, p, 64, p, None, None) == -3             # SEGF_ERR_WORKSPACE
            assert lib.segf_spatial_gate_bwd(dt, 2, 35, 64, p, 64, None, p, 64, p, p, p, p, 64, p, p, None, None) == -3
        assert t.kernels == []
    with hip.trace(dry_run=True) as t:
        assert lib.segf_gated_mul_fwd(7, 70, 64, p, 64, p, 64, p, 64, None) == -2                                   # SEGF_ERR_DTYPE
    assert t.kernels == []
