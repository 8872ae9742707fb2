"""Time the CrossFormer group attention (segf_group_attention_fwd / _bwd, csrc/attention_group.hip) at the four stage shapes of
crossformer_small at 512 x 512, batch 32, SDA and LDA, against the kernel's byte roofline.
Usage: python tools/bench_group_attention.py [--out profiles/group_attention.md] [--iters 50] [--dtype bf16|fp32] [--batch 32]

Bytes are the algorithmic ones: forward reads qkv (3 C per token) and writes o (C) + lse (4 bytes per token and head); backward reads
qkv, dO and lse and writes dq | dk | dv (7 C per token).  NOT counted: the bias and its gradient (heads x 49 x 49 floats) and the
backward's workspace -- one 49 x 49 fp32 slab (9.6 KB) per workgroup, up to 2048 of them = 19.7 MB, written by the backward kernel and
read back by the reduction (printed per row as `ws MB`, each way).  The fraction is against 8 TB/s (HBM3E peak, MI355X)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

# crossformer_small (crossformer.py:796-804) at 512 x 512: (map side, heads, interval)
STAGES = [(128, 3, 8), (64, 6, 4), (32, 12, 2), (16, 24, 1)]
G = 7
PEAK_BW = 8.0e12


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
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
    es = 2 if a.dtype == 'bf16' else 4
    B = a.batch
    lines = ['| map (B, H, W, heads) | mode | fwd us | fwd MB | fwd TB/s | of 8 TB/s | bwd us | bwd MB | bwd TB/s | of 8 TB/s | ws MB |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    g = torch.Generator().manual_seed(0)
    scale = 32 ** -0.5
    for side, heads, interval in STAGES:
        rows, C = B * side * side, heads * 32
        qkv = torch.randn(rows, 3 * C, generator=g).to(dtype).cuda()
        do = torch.randn(rows, C, generator=g).to(dtype).cuda()
        bias = (torch.randn(heads, G * G, G * G, generator=g) * 0.5).cuda()
        for lda in (False, True):
            args = (B, side, side, heads, G, interval, lda, scale)
            _, lse = hip.group_attention_fwd(qkv, bias, *args)
            t_f = timed(lambda: hip.group_attention_fwd(qkv, bias, *args), a.iters)
            t_b = timed(lambda: hip.group_attention_bwd(qkv, bias, do, lse, *args), a.iters)
            by_f = rows * (4 * C * es + 4 * heads)
            ws_mb = hip.lib().segf_group_attention_bwd_ws(B, side, side, heads, 32, G, interval, int(lda)) * 4 / 1e6
            by_b = rows * (7 * C * es + 4 * heads)
            bw_f, bw_b = by_f / (t_f * 1e-6), by_b / (t_b * 1e-6)
            lines.append(f'| {B}, {side}, {side}, {heads} | {"LDA I=%d" % interval if lda else "SDA"} | {t_f:.1f} | {by_f / 1e6:.1f} | '
                         f'{bw_f / 1e12:.2f} | {bw_f / PEAK_BW:.2f} | {t_b:.1f} | {by_b / 1e6:.1f} | {bw_b / 1e12:.2f} | {bw_b / PEAK_BW:.2f} | {ws_mb:.1f} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(f'# CrossFormer group attention (csrc/attention_group.hip), {a.dtype}, MI355X: tools/bench_group_attention.py\n\n' + text)


if __name__ == '__main__':
    main()
