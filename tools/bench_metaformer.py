"""Time the four MetaFormer kernels (csrc/metaformer.hip: StarReLU and the residual scale, forward and backward) at the stage shapes of
convformer_s18 and convformer_b36 for 512 x 512 images at batch 64 (maps 128^2, 64^2, 32^2, 16^2), bf16, against their byte counts and
against the copy bandwidth of the same box (the `copy (1R + 1W)` yardstick of tools/membw.py, measured here in the same process on the
same buffer size).
Usage: python tools/bench_metaformer.py [--out profiles/convformer.md] [--iters 30] [--batch 64]

StarReLU runs at two widths per stage: 2 C behind SepConv's first Linear and 4 C behind the MLP's; the residual scale exists in stages 3
and 4 only, at width C.  Bytes counted per kernel: the [M, cols] operands it reads and writes (2 bytes each); the parameters and the
per-workgroup partial sums are left out (below 1 % at every shape)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

MODELS = {'convformer_s18': (64, 128, 320, 512), 'convformer_b36': (128, 256, 512, 768)}
MAPS = (128, 64, 32, 16)
# (reads, writes) of [M, cols] operands
TRAFFIC = {'star_relu fwd': (1, 1), 'star_relu bwd': (2, 1), 'col_scale fwd': (1, 1), 'col_scale bwd': (2, 1)}


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
    s, b = torch.tensor([1.1], device='cuda'), torch.tensor([-0.1], device='cuda')
    for model, dims in MODELS.items():
        for stage, (side, C) in enumerate(zip(MAPS, dims)):
            M = B * side * side
            for cols in (2 * C, 4 * C, C):
                if cols == C and stage < 2:
                    continue                                    # no residual scale in stages 1 and 2
                u = torch.randn(M, cols, device='cuda', dtype=torch.bfloat16)
                dy = torch.randn(M, cols, device='cuda', dtype=torch.bfloat16)
                if cols == C:
                    sc = 1.0 + 0.1 * torch.randn(C, device='cuda')
                    fns = {'col_scale fwd': lambda: hip.colscale_fwd(u, sc), 'col_scale bwd': lambda: hip.colscale_bwd(dy, u, sc)}
                else:
                    fns = {'star_relu fwd': lambda: hip.starrelu_fwd(u, s, b), 'star_relu bwd': lambda: hip.starrelu_bwd(u, dy, s)}
                for name, fn in fns.items():
                    rd, wr = TRAFFIC[name]
                    byt = (rd + wr) * M * cols * 2
                    us = timed(fn, a.iters)
                    tbs = byt / (us * 1e-6) / 1e12
                    rows.append((model, stage + 1, side, cols, name, byt / 1e6, us, tbs, tbs / bw))
                    print(f'{model} stage {stage + 1} ({side}^2 x {cols}) {name}: {us:.1f} us, {tbs:.2f} TB/s = {100 * tbs / bw:.0f} % of copy',
                          flush=True)
                del u, dy
    lines = ['| model | stage | map | cols | kernel | MB moved | us | TB/s | of copy |', '|---|---|---|---|---|---|---|---|---|']
    for m, st, side, cols, name, mb, us, tbs, frac in rows:
        lines.append(f'| {m} | {st} | {side}^2 | {cols} | {name} | {mb:.1f} | {us:.1f} | {tbs:.2f} | {100 * frac:.0f} % |')
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(f'# MetaFormer kernels (csrc/metaformer.hip), bf16, batch {B}, 512 x 512 stage shapes, MI355X: tools/bench_metaformer.py\n\n'
                     f'Copy bandwidth of the same box in the same process (`b.copy_(a)`, 1R + 1W, the buffer of tools/membw.py): {bw:.2f} TB/s.\n'
                     f'The times include the allocation of the outputs and, for the backward passes, the finalize launch.\n\n' + text)


if __name__ == '__main__':
    main()
