#!/usr/bin/env python3
"""Multi-scale + flip sliding-window evaluation: the fused kernel (segf_msf_slide_argmax_confmat) against the bytes it must move,
against the unfused torch restatement on the same GPU, and as a share of one full slide-msf step of MiT-B0 + SegFormerHead.  One
process, one JSON line.

    python tools/bench_msf_slide.py [--eval-dtype fp32] [--iters 50] [--steps 5] [--runs 3] [--window-batch 32]

Two configurations, the published ones, both with the six default scales and the flip (12 window sets): Cityscapes (B = 1,
1024 x 2048, crop 1024, stride 768, 19 classes) and ADE20K (B = 8, 512 x 683, crop 512, stride 341, 150 classes); stride-4 head
outputs.  Per configuration, every time as [min, median, max] of --runs runs:
  kernel_ms / kernel_gbs   device-event time of the kernel alone and its rate over the bytes it MUST read and write (every window map
                           once, the labels once, the two count matrices), for bf16 and fp32 maps;
  torch_ms / torch_peak_mb the same result from torch ops: per set and window NHWC -> NCHW, F.interpolate to the crop, add_ into the
                           [B, C, Hs, Ws] accumulator, divide by the count map, flip, F.interpolate to the label size, softmax, add;
                           then argmax and the library's counting of explicit pairs (segf_confmat_pairs); the peak of the allocator
                           above the inputs while it runs;
  pred_agreement           share of the pixels at which the two predictions agree (they differ only at fp32 near-ties);
  step_ms / kernel_share   engine.evaluate_msf_slide per batch (resizes, slicing the windows, the forwards in chunks of
                           --window-batch, the kernel; host clock around a synchronised loop) and the kernel's share of it."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import SegmentationModel, engine, hip  # noqa: E402

CONFIGS = (dict(name='cityscapes', batch=1, H=1024, W=2048, crop=1024, stride=768, classes=19),
           dict(name='ade20k', batch=8, H=512, W=683, crop=512, stride=341, classes=150))


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # ms


def spread(vals, nd=3):
    return [round(min(vals), nd), round(statistics.median(vals), nd), round(max(vals), nd)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eval-dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--window-batch', type=int, default=32)
    ap.add_argument('--configs', nargs='+', default=[c['name'] for c in CONFIGS], choices=[c['name'] for c in CONFIGS])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_msf_slide.py measures on the GPU'
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    scales = engine.MSF_SCALES
    out = {'bench': 'msf_slide_eval', 'eval_dtype': a.eval_dtype, 'scales': list(scales), 'flip': True, 'runs': a.runs, 'cases': []}
    for cfg in (c for c in CONFIGS if c['name'] in a.configs):
        B, H, W, C = cfg['batch'], cfg['H'], cfg['W'], cfg['classes']
        geoms = []                                                                  # (size, crop, stride, origins, flip) per set
        for size in engine.msf_sizes(H, W, scales):
            crop, stride, origins = engine.slide_windows(size[0], size[1], cfg['crop'], cfg['stride'])
            geoms += [(size, crop, stride, origins, 0), (size, crop, stride, origins, 1)]
        flips = [f for *_, f in geoms]
        case = dict(cfg, sets=len(geoms), windows_per_image=sum(len(o) for _, _, _, o, _ in geoms))
        target = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        target[:, :8] = 255
        mat = torch.zeros((C, C), dtype=torch.int64, device=dev)
        hist, flag = mat.clone(), torch.zeros(1, dtype=torch.int32, device=dev)
        pred = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
            rows = [(3 * torch.randn(B * len(o) * (ch // 4) * (cw // 4), C, device=dev, generator=g)).to(dt) for _, (ch, cw), _, o, _ in geoms]
            sets = [((r, ch // 4, cw // 4), size, (ch, cw), strd) for r, (size, (ch, cw), strd, _, _) in zip(rows, geoms)]
            nbytes = sum(r.numel() * r.element_size() for r in rows) + target.numel() * 8 + 2 * C * C * 8
            ms = [timeit(lambda: hip.msf_slide_argmax_confmat(sets, flips, B, C, H, W, target, 255, mat, hist, flag), a.iters)
                  for _ in range(a.runs)]
            case[f'kernel_ms_{name}'] = spread(ms, 4)
            case[f'kernel_gbs_{name}'] = round(nbytes / statistics.median(ms) / 1e6, 1)
            case[f'must_move_mb_{name}'] = round(nbytes / 1e6, 1)
            hip.msf_slide_argmax_confmat(sets, flips, B, C, H, W, None, 255, None, None, None, pred_out=pred)
            kept = {}

            def restated():
                S = None
                for r, (size, (ch, cw), _, origins, f) in zip(rows, geoms):
                    maps = r.view(B, len(origins), ch // 4, cw // 4, C)
                    acc = torch.zeros((B, C, size[0], size[1]), dtype=torch.float32, device=dev)
                    cnt = torch.zeros((1, 1, size[0], size[1]), dtype=torch.float32, device=dev)
                    for k, (y, x) in enumerate(origins):
                        z = F.interpolate(maps[:, k].float().permute(0, 3, 1, 2), size=(ch, cw), mode='bilinear', align_corners=False)
                        acc[:, :, y:y + ch, x:x + cw].add_(z)
                        cnt[:, :, y:y + ch, x:x + cw].add_(1)
                    acc.div_(cnt)
                    if f:
                        acc = acc.flip(3)
                    if tuple(size) != (H, W):
                        acc = F.interpolate(acc, size=(H, W), mode='bilinear', align_corners=False)
                    p = acc.softmax(1)
                    S = p if S is None else S.add_(p)
                kept['pred'] = S.argmax(1)
                hip.confmat_pairs(target.flatten(), kept['pred'].flatten(), C, 255, mat, hist, flag)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            case[f'torch_ms_{name}'] = spread([timeit(restated, max(2, a.iters // 5), warm=1) for _ in range(a.runs)], 3)
            case[f'torch_peak_mb_{name}'] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
            case[f'pred_agreement_{name}'] = round((kept['pred'] == pred).float().mean().item(), 6)
            del rows, sets, kept
            torch.cuda.empty_cache()
        # one full slide-msf step: resizes, slicing the windows, the forwards, the kernel
        model = SegmentationModel('MiT-B0', num_classes=C, seg_head='SegFormerHead').to(dev).eval()
        x = torch.randn(B, 3, H, W, device=dev, generator=g)
        args = types.SimpleNamespace(nb_classes=C, ignore_label=255, eval_dtype=a.eval_dtype)
        kw = dict(crop=cfg['crop'], stride=cfg['stride'], window_batch=a.window_batch)
        steps = []
        with contextlib.redirect_stdout(sys.stderr):                                # the logger's lines: stdout carries the JSON line only
            engine.evaluate_msf_slide(args, model, [(x, target)] * 2, dev, 1000, **kw)       # eager sightings, captures, first replays
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                engine.evaluate_msf_slide(args, model, [(x, target)] * a.steps, dev, 1000, **kw)
                torch.cuda.synchronize()
                steps.append((time.perf_counter() - t0) * 1e3 / a.steps)
        k = statistics.median(ms) if a.eval_dtype == 'fp32' else case['kernel_ms_bf16'][1]
        case.update(step_ms=spread(steps, 2), kernel_share=round(k / statistics.median(steps), 4))
        out['cases'].append(case)
        del model
        torch.cuda.empty_cache()
    out['fused_not_slower_than_torch'] = all(c[f'kernel_ms_{n}'][1] <= c[f'torch_ms_{n}'][1] for c in out['cases'] for n in ('bf16', 'fp32'))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
