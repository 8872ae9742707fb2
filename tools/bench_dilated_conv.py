"""Time the dilated 3x3 convolution (segf_conv3x3_dil: forward, data gradient, weight gradient; bf16) at the ASPP shapes, with and
without tap culling (SEGFAC_DILCONV_NO_CULL), next to segf_conv3x3 (the dense 3x3 convolution, dilation 1) at the same shapes.
Usage: python tools/bench_dilated_conv.py [--out profiles/dilated_conv.md] [--iters 50]

FLOPs are the EXECUTED ones of the culled form: per live tap, 2 * Cin * Cout for every pixel that reads inside the image through that
tap.  The matrix-rate fraction is against 2.5 PFLOP/s (dense bf16, MI355X)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

SHAPES = [(64, 16, 16, 256, 256), (64, 16, 16, 768, 256), (16, 32, 32, 512, 256)]      # (B, H, W, Cin, Cout)
RATES = (12, 24, 36)
PEAK = 2.5e15


def executed_flops(B, H, W, I, O, d):
    n = 0
    for tap in hip.conv3x3_dil_live_taps(H, W, d):
        ty, tx = tap // 3 - 1, tap % 3 - 1
        n += max(0, H - abs(ty) * d) * max(0, W - abs(tx) * d)
    return 2.0 * B * n * I * O


def timed(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    lines = ['| shape (B, H, W, Cin->Cout) | d | mode | culled us | all taps us | ratio | dense 3x3 us | executed GFLOP | of bf16 matrix rate |',
             '|---|---|---|---|---|---|---|---|---|']
    g = torch.Generator().manual_seed(0)
    for (B, H, W, I, O) in SHAPES:
        P = B * H * W
        x = torch.randn(P, I, generator=g).bfloat16().cuda()
        dy = torch.randn(P, O, generator=g).bfloat16().cuda()
        wm = (torch.randn(O, 9 * I, generator=g) / (9 * I) ** 0.5).bfloat16().cuda()
        wt = (torch.randn(I, 9 * O, generator=g) / (9 * O) ** 0.5).bfloat16().cuda()
        ops = {'fwd': (0, x, wm), 'dgrad': (1, dy, wt), 'wgrad': (2, x, dy)}
        dense = {}
        for name, (mode, p, q) in ops.items():
            kw = dict(split_k=hip.pick_splitk_conv3x3(I, O, P)) if mode == 2 else {}
            dense[name] = timed(lambda: hip.conv3x3(mode, p, q, B, H, W, I, O, **kw), a.iters)
        for d in RATES:
            fl = executed_flops(B, H, W, I, O, d)
            for name, (mode, p, q) in ops.items():
                t_c = timed(lambda: hip.conv3x3_dil(mode, p, q, B, H, W, I, O, d), a.iters)
                with hip.policy_override(dilconv_no_cull=1):
                    t_n = timed(lambda: hip.conv3x3_dil(mode, p, q, B, H, W, I, O, d), a.iters)
                lines.append(f'| {B}, {H}, {W}, {I}->{O} | {d} | {name} | {t_c:.1f} | {t_n:.1f} | {t_c / t_n:.2f} | {dense[name]:.1f} | '
                             f'{fl / 1e9:.2f} | {fl / (t_c * 1e-6) / PEAK:.3f} |')
                print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('# Dilated 3x3 convolution (csrc/conv_dilated.hip), bf16, MI355X: tools/bench_dilated_conv.py\n\n' + text)


if __name__ == '__main__':
    main()
