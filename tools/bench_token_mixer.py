"""Time the three CAS-ViT token-mixer kernel pairs (csrc/token_mixer.hip) at the four stage shapes of rcvit_s and rcvit_t for 512 x 512
images at batch 64 (maps 128^2, 64^2, 32^2, 16^2), bf16, against their byte counts and against the copy bandwidth of the same box
(the `copy (1R + 1W)` yardstick of tools/membw.py, measured here in the same process on the same buffer size).
Usage: python tools/bench_token_mixer.py [--out profiles/token_mixer.md] [--iters 30] [--batch 64]

Bytes counted per kernel: the [M, C] operands it reads and writes (2 bytes each) plus the fp32 s vector of the spatial gate; the [B, C]
gates, pooled sums and the per-workgroup partial sums are left out (below 1 % at every shape)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

MODELS = {'rcvit_s': (48, 64, 128, 256), 'rcvit_t': (96, 128, 256, 512)}
MAPS = (128, 64, 32, 16)
# (reads, writes) of [M, C] operands
TRAFFIC = {'spatial_gate fwd': (2, 1), 'spatial_gate bwd': (3, 2), 'channel_gate_mix fwd': (2, 1), 'channel_gate_mix bwd': (3, 2),
           'gated_mul fwd': (2, 1), 'gated_mul bwd': (3, 2)}


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def copy_bandwidth(iters):
    """TB/s of b.copy_(a) on the buffer of tools/membw.py (a [64 * 128 * 128, 768] bf16 activation)."""
    n = 1610612736 // 2
    a = torch.empty(n, dtype=torch.bfloat16, device='cuda')
    b = torch.empty_like(a)
    a.zero_()
    us = timed(lambda: b.copy_(a), max(iters // 3, 5))
    return 4 * n / (us * 1e-6) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args()
    B = a.batch
    bw = copy_bandwidth(a.iters)
    print(f'copy bandwidth (1R + 1W): {bw:.2f} TB/s', flush=True)
    rows = []
    done = set()
    for model, dims in MODELS.items():
        for stage, (side, C) in enumerate(zip(MAPS, dims)):
            HW, M = side * side, B * side * side
            g = torch.Generator(device='cuda').manual_seed(stage)
            x, k, dy = (torch.randn(M, C, generator=g, device='cuda').to(torch.bfloat16) for _ in range(3))
            r = torch.relu(torch.randn(M, C, generator=g, device='cuda')).to(torch.bfloat16)
            w = torch.randn(C, generator=g, device='cuda') / C ** 0.5
            gq, gk, dpool = (torch.rand(B, C, generator=g, device='cuda') for _ in range(3))
            _, s, _ = hip.spatial_gate_fwd(x, r, w, B, HW)
            fns = {'spatial_gate fwd': lambda: hip.spatial_gate_fwd(x, r, w, B, HW),
                   'spatial_gate bwd': lambda: hip.spatial_gate_bwd(dy, dpool, x, r, s, w, B, HW),
                   'channel_gate_mix fwd': lambda: hip.channel_gate_mix_fwd(x, k, gq, gk, B, HW),
                   'channel_gate_mix bwd': lambda: hip.channel_gate_mix_bwd(dy, x, k, gq, gk, B, HW),
                   'gated_mul fwd': lambda: hip.gated_mul_fwd(x, k),
                   'gated_mul bwd': lambda: hip.gated_mul_bwd(dy, x, k)}
            for name, fn in fns.items():
                rd, wr = TRAFFIC[name]
                byt = (rd + wr) * M * C * 2 + (4 * M if name.startswith('spatial') else 0)
                us = timed(fn, a.iters)
                tbs = byt / (us * 1e-6) / 1e12
                rows.append((model, stage + 1, side, C, name, byt / 1e6, us, tbs, tbs / bw))
                print(f'{model} stage {stage + 1} ({side}^2 x {C}) {name}: {us:.1f} us, {tbs:.2f} TB/s = {100 * tbs / bw:.0f} % of copy', flush=True)
            del x, k, dy, r
    lines = ['| model | stage | map | C | kernel | MB moved | us | TB/s | of copy |', '|---|---|---|---|---|---|---|---|---|']
    for m, st, side, C, name, mb, us, tbs, frac in rows:
        lines.append(f'| {m} | {st} | {side}^2 | {C} | {name} | {mb:.1f} | {us:.1f} | {tbs:.2f} | {100 * frac:.0f} % |')
    text = '\n'.join(lines) + '\n'
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(f'# Token-mixer kernels (csrc/token_mixer.hip), bf16, batch {B}, 512 x 512 stage shapes, MI355X: tools/bench_token_mixer.py\n\n'
                     f'Copy bandwidth of the same box in the same process (`b.copy_(a)`, 1R + 1W, the buffer of tools/membw.py): {bw:.2f} TB/s.\n'
                     f'The times include the allocation of the outputs and, where a kernel sums over rows, its finalize launch.\n\n' + text)


if __name__ == '__main__':
    main()
