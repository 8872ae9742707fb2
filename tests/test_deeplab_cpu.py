"""CPU-only checks of the DeepLabV3 head: state_dict keys against the reference's inventory (recorded in the fixture by
tools/make_deeplab_goldens.py), the factory rule, the CLI, and the host side of the dilated-convolution entry points."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

from tools.make_deeplab_goldens import head_state_dict, load_inventory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = 'e2e_deeplabv3_mitb0_416x448.npz'


def _with_input_width(inventory, c1):
    """The reference head's inventory for another ASPP input width: only the five branch convolutions see it."""
    out = []
    for k, s in inventory:
        if k.endswith(('aspp.b0.0.weight', 'aspp.b1.block.0.weight', 'aspp.b2.block.0.weight', 'aspp.b3.block.0.weight',
                       'aspp.b4.gap.1.weight')):
            s = (s[0], c1) + tuple(s[2:])
        out.append((k, s))
    return out


@pytest.mark.parametrize('backbone,c1', [('MiT-B0', 256), ('ConvNeXt', 768), ('MobileNetV2', 320)])
def test_state_dict_matches_the_reference_inventory(golden_dir, backbone, c1):
    from segmentation_factory_amd import SegmentationModel
    g = np.load(os.path.join(golden_dir, FIXTURE))
    inv = load_inventory(g)
    assert len(inv) == 44 and inv[0] == ('decode_head.head.aspp.b0.0.weight', (256, 256, 1, 1))
    assert inv[-2:] == [('decode_head.head.block.4.weight', (7, 256, 1, 1)), ('decode_head.head.block.4.bias', (7,))]
    m = SegmentationModel(backbone, num_classes=7, seg_head='deeplabv3')
    assert m.backbone.channels[-1] == c1
    head = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k.startswith('decode_head.')]
    assert head == _with_input_width(inv, c1)                       # key ORDER and shapes
    if backbone == 'MiT-B0':
        sd = head_state_dict(inv, int(g['head_seed']))              # the generator still draws what the fixture was made with
        norms = [sd[k].double().norm().item() for k, _ in inv]
        assert np.allclose(norms, g['head_weight_norms'], rtol=1e-12, atol=0)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith('backbone.') for k in missing)
    # any spelling that contains 'deeplabv3' matches (models/build_models.py:47)
    assert type(SegmentationModel(backbone, num_classes=7, seg_head='DeepLabV3').decode_head).__name__ == 'DeepLabV3'


def test_aux_and_fp8_are_refused():
    from segmentation_factory_amd import SegmentationModel
    with pytest.raises(NotImplementedError, match='aux'):
        SegmentationModel('MiT-B0', num_classes=7, seg_head='deeplabv3', aux_for_deeplab=True)
    m = SegmentationModel('MiT-B0', num_classes=7, seg_head='deeplabv3')
    with pytest.raises(ValueError, match='no fp8-capable layers'):
        m.set_fp8(True)
    with pytest.raises(KeyError):
        SegmentationModel('MiT-B0', num_classes=7, seg_head='NoSuchHead')


def test_train_gpu_accepts_the_head():
    spec = importlib.util.spec_from_file_location('train_gpu_cli_deeplab', os.path.join(ROOT, 'train_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.ArgumentParser(parents=[mod.get_args_parser()]).parse_args(['--heads', 'deeplabv3'])
    assert args.heads == 'deeplabv3'
    assert argparse.ArgumentParser(parents=[mod.get_args_parser()]).parse_args([]).heads == 'SegFormerHead'


GPU_SHAPES = [(1, 1, 1, 8, 8, 12), (2, 13, 14, 40, 24, 12), (2, 16, 16, 256, 256, 24), (1, 40, 28, 72, 264, 36),
              (3, 37, 41, 320, 256, 12), (2, 9, 11, 64, 32, 2), (2, 16, 16, 256, 256, 12), (2, 16, 16, 256, 256, 36)]


def test_dilated_conv_supported_is_a_dry_call():
    from segmentation_factory_amd import hip
    for dtype in (torch.float32, torch.bfloat16):
        for B, H, W, I, O, d in GPU_SHAPES:
            for mode in (0, 1, 2):
                assert hip.conv3x3_dil_supported(dtype, mode, B, H, W, I, O, d), (dtype, mode, B, H, W, I, O, d)
        assert not hip.conv3x3_dil_supported(dtype, 0, 2, 13, 14, 44, 24, 12)          # Cin not a multiple of 8
        assert not hip.conv3x3_dil_supported(dtype, 0, 2, 13, 14, 40, 20, 12)          # Cout not a multiple of 8
        assert not hip.conv3x3_dil_supported(dtype, 0, 2, 13, 14, 40, 24, 0)           # dilation 0
        assert not hip.conv3x3_dil_supported(dtype, 3, 2, 13, 14, 40, 24, 12)          # no such mode
    assert not hip.conv3x3_dil_supported(torch.float16, 0, 2, 13, 14, 40, 24, 12)
    # the launch path refuses what `supported` refuses, and shapes whose element offsets leave 32 bits -- as dry runs, nothing launched
    ph = 0x7f0000000000
    with hip.trace(dry_run=True) as t:
        assert hip.lib().segf_conv3x3_dil(hip.BF16, 0, 2, 13, 14, 44, 24, 12, ph, 48, ph, 396, ph, 24, 1, None, None) == hip.ERR_SHAPE
        assert hip.lib().segf_conv3x3_dil(hip.BF16, 0, 4096, 256, 256, 64, 64, 12, ph, 64, ph, 576, ph, 64, 1, None, None) == hip.ERR_SHAPE
        assert hip.lib().segf_conv3x3_dil(hip.BF16, 0, 2, 16, 16, 256, 256, 12, ph, 1280, ph, 2304, ph, 256, 1, None, None) == 0
        assert hip.lib().segf_conv3x3_dil(hip.F32, 2, 2, 16, 16, 256, 256, 12, ph, 256, ph, 256, ph, 2304, 4, ph, None) == 0
    assert t.kernels == ['conv3x3_dil_kernel<T>', 'conv3x3_dil_wgrad_kernel<T>', 'conv3x3_dil_reduce_kernel'], t.kernels
    assert hip.pick_splitk_conv3x3_dil(1, 1, 1, 8, 8, 12) == 1
    assert 1 <= hip.pick_splitk_conv3x3_dil(64, 16, 16, 256, 256, 24) <= 64


def test_live_tap_list():
    from segmentation_factory_amd import hip
    assert hip.conv3x3_dil_live_taps(16, 16, 12) == list(range(9))
    assert hip.conv3x3_dil_live_taps(16, 16, 24) == [4]
    assert hip.conv3x3_dil_live_taps(40, 28, 36) == [1, 4, 7]           # the vertical ones
    assert hip.conv3x3_dil_live_taps(1, 1, 12) == [4]
    assert hip.conv3x3_dil_live_taps(13, 14, 12) == list(range(9)) and hip.conv3x3_dil_live_taps(13, 14, 13) == [3, 4, 5]
    with pytest.raises(ValueError):
        hip.conv3x3_dil_live_taps(16, 16, 0)
    assert hip.policy('dilconv_no_cull') == 0
