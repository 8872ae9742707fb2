"""CrossFormer backbones, the parts that need no GPU: the group-to-token map against the reference's pad / reshape / permute sequence,
the module surface (names, state_dict inventory, channels), the small-map rule and the C ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# (B, H, W, heads, G, interval, lda): the kernel shape list of tests/test_crossformer_gpu.py
KERNEL_SHAPES = [
    (1, 7, 7, 2, 7, 1, False),          # one full group, no padding
    (2, 9, 10, 2, 7, 1, False),         # padding on both sides, groups with two real rows
    (1, 16, 20, 4, 7, 2, True),         # interval gather, padding to 28 x 28
    (1, 57, 8, 2, 7, 8, True),          # a second region whose groups are mostly or wholly padding
    (1, 4, 6, 8, 6, 1, False),          # small-map rule, N = 36
    (3, 2, 3, 16, 3, 1, False),         # small-map rule, N = 9, 16 heads in a 512-wide row
    (1, 7, 8, 2, 8, 1, False),          # the largest tile, N = 64
    (2, 8, 10, 16, 7, 1, True),         # I = 1, stage 4 of the large fixture
]


# Shapes at which a backward workgroup walks SEVERAL groups (the kernel gives one workgroup ceil(groups / (2048 / heads)) of them: 2 and 3
# here, as every training shape has), with the padding pattern changing along the walk
MULTI_GROUP_SHAPES = [
    (8, 84, 90, 2, 7, 1, False),        # 1248 groups of 2 heads: two per workgroup; every 13th group has six real columns
    (16, 60, 100, 2, 7, 4, True),       # 3072 groups: three per workgroup; last region: one real row, four real columns
]


def reference_token_map(H, W, G, I, lda):
    """arange(H * W) pushed through crossformer.py:282-313 (pad right / bottom, reshape, permute), -1 in the padding."""
    x = torch.arange(H * W, dtype=torch.int64).view(1, H, W, 1)
    size_div = I * G if lda else G
    pad_r = (size_div - W % size_div) % size_div
    pad_b = (size_div - H % size_div) % size_div
    x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b), value=-1)
    _, Hp, Wp, _ = x.shape
    if not lda:
        x = x.reshape(1, Hp // G, G, Wp // G, G, 1).permute(0, 1, 3, 2, 4, 5).contiguous()
        return x.reshape(Hp * Wp // G ** 2, G ** 2)
    Rh, Rw = Hp // (G * I), Wp // (G * I)
    x = x.reshape(1, Rh, G, I, Rw, G, I, 1).permute(0, 1, 4, 3, 6, 2, 5, 7).contiguous()
    return x.reshape(Rh * Rw * I * I, G * G)


@pytest.mark.parametrize('shape', KERNEL_SHAPES + MULTI_GROUP_SHAPES, ids=[str(s) for s in KERNEL_SHAPES + MULTI_GROUP_SHAPES])
def test_group_token_index_is_the_reference_map(shape):
    from segmentation_factory_amd import functional as Fh
    _, H, W, _, G, I, lda = shape
    got = Fh.group_token_index(H, W, G, I, lda)
    ref = reference_token_map(H, W, G, I, lda)
    assert got.shape == ref.shape and torch.equal(got, ref)
    real = got[got >= 0]
    assert torch.equal(torch.sort(real).values, torch.arange(H * W))          # every real token exactly once


@pytest.mark.parametrize('name', ['crossformer_tiny', 'crossformer_small', 'crossformer_base', 'crossformer_large'])
def test_factories_build(name):
    from segmentation_factory_amd import SegmentationModel
    m = SegmentationModel(name, num_classes=7, seg_head='SegFormerHead')
    E = {'tiny': 64, 'small': 96, 'base': 96, 'large': 128}[name.split('_')[1]]
    assert m.backbone.channels == [E, 2 * E, 4 * E, 8 * E]
    width = m.decode_head.state_dict()['linear_pred.weight'].shape[1]
    assert width == (128 if name in ('crossformer_tiny', 'crossformer_small') else 768)


def test_tiny_state_dict_is_the_reference_inventory(golden_dir):
    from segmentation_factory_amd import SegmentationModel
    from tools.make_crossformer_goldens import load_inventory
    g = np.load(os.path.join(golden_dir, 'e2e_crossformer_tiny_256x320.npz'))
    inv = load_inventory(g)
    m = SegmentationModel('crossformer_tiny', num_classes=int(g['nc']), seg_head='SegFormerHead')
    assert m.backbone.channels == [64, 128, 256, 512]
    mine = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert sorted(mine) == sorted(inv)
    assert [k for k, _ in mine if k.startswith('backbone.')] == [k for k, _ in inv if k.startswith('backbone.')]       # and the order
    keys = {k for k, _ in mine}
    for k in ('backbone.patch_embed.projs.0.weight', 'backbone.patch_embed.norm.bias', 'backbone.layers.2.blocks.1.attn.pos.pos_proj.weight',
              'backbone.layers.2.blocks.1.attn.pos.pos3.2.bias', 'backbone.layers.0.downsample.reductions.0.weight',
              'backbone.layers.0.downsample.norm.weight', 'backbone.layers.3.blocks.5.mlp.fc2.bias'):
        assert k in keys, k
    assert not any(k.startswith('backbone.layers.3.downsample') for k in keys)


def test_init_follows_the_reference():
    from segmentation_factory_amd import backbones
    torch.manual_seed(0)
    m = backbones.crossformer_tiny()
    blk = m.layers[2].blocks[1]
    assert float(blk.attn.qkv.weight.detach().abs().max()) <= 2.0 and abs(float(blk.attn.qkv.weight.detach().std()) - 0.02) < 2e-3
    assert float(blk.attn.qkv.bias.detach().abs().max()) > 0            # Linear biases keep torch's default initialisation
    assert torch.equal(blk.norm1.weight, torch.ones(256)) and torch.equal(blk.norm1.bias, torch.zeros(256))
    assert blk.attn.pos.pos_dim == 256 // 16
    rates = [b.drop_prob for st in m.layers for b in st.blocks]
    assert np.allclose(rates, torch.linspace(0, 0.1, 16).tolist())
    assert [b.lsda_flag for b in m.layers[2].blocks] == [0, 1] * 4 and [b.interval for b in m.layers[2].blocks] == [2] * 8


def test_crossformerpp_is_still_missing():
    from segmentation_factory_amd import SegmentationModel
    with pytest.raises(KeyError):
        SegmentationModel('crossformerpp_base', num_classes=7, seg_head='SegFormerHead')


def test_small_map_rule_is_sticky():
    """crossformer.py:263-269: a map with min(H, W) <= group_size turns the block into an SDA block for good."""
    from segmentation_factory_amd import backbones
    blk = backbones.crossformer_tiny().layers[2].blocks[1]
    assert blk.lsda_flag == 1 and blk.grouping(16, 20) == (7, 2, True)
    assert blk.grouping(6, 8) == (8, 2, False)                 # one group of side max(H, W)
    assert blk.grouping(16, 20) == (7, 2, False) and blk.lsda_flag == 0


def test_position_bias_tables_and_gather_backward():
    """DynamicPosBias on the CPU: the gathered bias equals pos[relative_position_index] of crossformer.py:129-150, and the fixed-order
    backward of the gather equals autograd's."""
    from segmentation_factory_amd import backbones
    torch.manual_seed(1)
    pos = backbones.DynamicPosBias(64 // 4, 2)
    for G in (7, 3):
        offsets, idx, pairs = pos.tables(G, 'cpu')
        h = torch.arange(1 - G, G)
        biases = torch.stack(torch.meshgrid([h, h], indexing='ij')).flatten(1).transpose(0, 1).contiguous().float()
        assert torch.equal(offsets, biases)
        c = torch.stack(torch.meshgrid([torch.arange(G), torch.arange(G)], indexing='ij')).flatten(1)
        rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += G - 1
        rel[:, :, 1] += G - 1
        rel[:, :, 0] *= 2 * G - 1
        assert torch.equal(idx, rel.sum(-1).view(-1))
        table = torch.randn((2 * G - 1) ** 2, 2, dtype=torch.float64, requires_grad=True)
        w = torch.randn(2, G * G, G * G, dtype=torch.float64)
        ref = table[idx].view(G * G, G * G, -1).permute(2, 0, 1)
        got = backbones._BiasGatherFn.apply(table, idx, pairs, G * G)
        assert torch.equal(got, ref)
        g_ref, = torch.autograd.grad((ref * w).sum(), table)
        g_got, = torch.autograd.grad((got * w).sum(), table)
        assert torch.allclose(g_got, g_ref, rtol=1e-12, atol=1e-12)
    b = pos.bias(7, 'cpu')
    assert b.shape == (2, 49, 49) and b.dtype == torch.float32 and b.requires_grad


def test_header_declares_the_group_attention_entries():
    from segmentation_factory_amd import hip
    with open(hip.HEADER_PATH) as fh:
        text = fh.read()
    for name in ('segf_group_attention_fwd', 'segf_group_attention_bwd', 'segf_group_attention_bwd_ws', 'segf_group_attention_supported'):
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in hip.exported_symbols()


def test_backward_workspace_counts_the_groups_per_workgroup():
    """segf_group_attention_bwd_ws (host arithmetic): one N x N slab per workgroup and head, a workgroup per ceil(groups / (2048 / heads))
    groups that hold a real token -- one group each at the small kernel shapes, two and three at MULTI_GROUP_SHAPES."""
    from segmentation_factory_amd import hip
    lib = hip.lib()
    per_wg = {}
    for B, H, W, heads, G, I, lda in KERNEL_SHAPES + MULTI_GROUP_SHAPES:
        from segmentation_factory_amd import functional as Fh
        idx = Fh.group_token_index(H, W, G, I, lda)
        groups = B * int((idx >= 0).any(1).sum())
        ipb = -(-groups // max(2048 // heads, 1))
        chunks = -(-groups // ipb)
        assert lib.segf_group_attention_bwd_ws(B, H, W, heads, 32, G, I, int(lda)) == chunks * heads * G ** 4
        per_wg[(B, H, W)] = ipb
    assert per_wg[(8, 84, 90)] == 2 and per_wg[(16, 60, 100)] == 3 and per_wg[(2, 8, 10)] == 1
    assert lib.segf_group_attention_bwd_ws(1, 9, 3, 2, 32, 9, 1, 0) == 0


def test_drop_path_scales_two_draws_per_block():
    """CrossFormer._drop_path_scales with a given keep mask: a block with rate 0 draws nothing, every other block gets rows 2k and 2k + 1
    of keep / (1 - rate) for its attention and MLP branches; eval mode draws nothing."""
    from segmentation_factory_amd import backbones
    m = backbones.crossformer_tiny().train()
    rates = [b.drop_prob for b in m._blocks()]
    assert rates[0] == 0 and all(r > 0 for r in rates[1:])
    keep = (torch.arange(30 * 2).view(30, 2) % 3 != 0).float()
    m.stochastic_override = {'drop_path': keep}
    sc = m._drop_path_scales(2, 'cpu')
    assert len(sc) == 16 and sc[0] == (None, None)
    for k, (r, (a, b)) in enumerate(zip(rates[1:], sc[1:])):
        assert torch.allclose(a, keep[2 * k] / (1 - r)) and torch.allclose(b, keep[2 * k + 1] / (1 - r))
    assert m.eval()._drop_path_scales(2, 'cpu') == [(None, None)] * 16
