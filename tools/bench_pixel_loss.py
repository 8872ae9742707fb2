"""Time the per-pixel loss kernels (segf_pixel_loss_fwd / _bwd, csrc/loss_pixel.hip) at the cfg2 head shape -- 150 classes, 128 x 128
-> 512 x 512, bf16 rows of 152 columns, batch 32 -- beside the existing CE + Dice pair with dice = 0 at the same shape in the same process.
Usage: python tools/bench_pixel_loss.py [--out profiles/pixel_loss.md] [--iters 50] [--batch 32] [--low 128]
                                        [--only ohem_thresh|ohem_topk|focal|ce_dice]
--low: edge of the low-resolution map, 512 / low in {2, 4, 8}.  At 128 (ratio 4, the default) the CE + Dice row runs the band kernels; at 256
and 64 it runs ce_dice_fwd_cells16_kernel / ce_dice_bwd_cells8_kernel, and the pixel rows their cell kernels at that ratio.

Rows: OHEM in the threshold branch (random logits: most pixels are hard, the eight selection kernels and the two top-k reductions are
launched and return at once), OHEM in the top-k branch (one class per image raised by 9: few pixels are hard, the radix select and the
reductions run over the 4-byte-per-pixel CE map), focal (0.25, 2), and ce_dice forward + backward with dice = 0.  HIP events around
`iters` back-to-back launches; forward (selection included) and backward are timed separately."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

C, LD, LOW, FULL, IGNORE = 150, 152, 128, 512, 255
THETA = float(-torch.log(torch.tensor(0.7, dtype=torch.float)))


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


def make_inputs(B, low, confident):
    g = torch.Generator(device='cuda').manual_seed(1 if confident else 0)
    wide = torch.zeros(B * low * low, LD, dtype=torch.bfloat16, device='cuda')
    lo = torch.randn(B, low, low, C, generator=g, device='cuda')
    t = torch.randint(0, C, (B, FULL, FULL), generator=g, device='cuda')
    if confident:
        kb = torch.randint(0, C, (B,), generator=g, device='cuda')
        lo[torch.arange(B, device='cuda'), :, :, kb] += 9.0
        other = torch.rand(B, FULL, FULL, generator=g, device='cuda') < 0.01
        t = torch.where(other, t, kb[:, None, None].expand(B, FULL, FULL))
    t[:, :8] = IGNORE
    t[torch.rand(B, FULL, FULL, generator=g, device='cuda') < 0.02] = IGNORE
    wide[:, :C] = lo.reshape(-1, C).to(torch.bfloat16)
    return wide[:, :C], t.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--only', default='')
    ap.add_argument('--low', type=int, default=LOW, choices=(64, 128, 256))
    a = ap.parse_args()
    B, low = a.batch, a.low
    geom = (B, C, low, low, FULL, FULL)
    go = torch.ones(1, device='cuda')
    rows = []

    def pixel(name, confident, mode, p0, p1):
        if a.only and a.only != name:
            return
        x, t = make_inputs(B, low, confident)
        args = (x, *geom, t, IGNORE, None, mode, p0, p1, 1)
        loss, ce_map, state = hip.pixel_loss_fwd(*args)
        info = state[:8].cpu().tolist()
        t_f = timed(lambda: hip.pixel_loss_fwd(*args), a.iters)
        t_b = timed(lambda: hip.pixel_loss_bwd(*args, ce_map, state, go), a.iters)
        note = f'loss {loss.item():.4f}' + (f', n_min {info[1]}, n_hard {info[2]}, used_topk {info[5]}' if mode == hip.PIXEL_OHEM else '')
        rows.append((name, t_f, t_b, note))
        print(f'{name}: fwd {t_f:.1f} us, bwd {t_b:.1f} us ({note})', flush=True)

    pixel('ohem_thresh', False, hip.PIXEL_OHEM, THETA, 0.0)
    pixel('ohem_topk', True, hip.PIXEL_OHEM, THETA, 0.0)
    pixel('focal', False, hip.PIXEL_FOCAL, 0.25, 2.0)
    if not a.only or a.only == 'ce_dice':
        x, t = make_inputs(B, low, False)
        loss, stats, lse = hip.ce_dice_fwd(x, *geom, t, IGNORE, None, 0, want_lse=True)
        t_f = timed(lambda: hip.ce_dice_fwd(x, *geom, t, IGNORE, None, 0, want_lse=True), a.iters)
        t_b = timed(lambda: hip.ce_dice_bwd(x, *geom, t, IGNORE, None, 0, stats, go, lse=lse), a.iters)
        rows.append(('ce_dice (dice = 0)', t_f, t_b, f'loss {loss[0].item():.4f}'))
        print(f'ce_dice: fwd {t_f:.1f} us, bwd {t_b:.1f} us', flush=True)
    base = next((f + b for n, f, b, _ in rows if n.startswith('ce_dice')), None)
    lines = ['| loss | fwd us | bwd us | fwd + bwd us | per image us | vs ce_dice pair | note |', '|---|---|---|---|---|---|---|']
    for n, f, b, note in rows:
        lines.append(f'| {n} | {f:.1f} | {b:.1f} | {f + b:.1f} | {(f + b) / B:.1f} | {"%.2f x" % ((f + b) / base) if base else "-"} | {note} |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(f'# Per-pixel losses (csrc/loss_pixel.hip) at C = {C}, {low}^2 -> {FULL}^2, bf16, batch {B}, MI355X: '
                     f'tools/bench_pixel_loss.py\n\n' + text)


if __name__ == '__main__':
    main()
