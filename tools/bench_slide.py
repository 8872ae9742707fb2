#!/usr/bin/env python3
"""Sliding-window evaluation: the fused kernel (segf_slide_argmax_confmat) against the bytes it must move, against the unfused torch
restatement on the same GPU, and as a share of one full sliding-window step of MiT-B0 + SegFormerHead.  One process, one JSON line.

    python tools/bench_slide.py [--eval-dtype fp32] [--iters 200] [--steps 20]

Two configurations, the published ones: Cityscapes (B = 1, 1024 x 2048, crop 1024, stride 768, 19 classes) and ADE20K (B = 8,
512 x 683, crop 512, stride 341, 150 classes); stride-4 head outputs.  Per configuration:
  kernel_ms / kernel_gbs   device-event time of the kernel alone and its rate over the bytes it MUST read and write (every window map
                           once, the labels once, the two count matrices), for bf16 and fp32 maps;
  torch_ms / torch_peak_mb the same result from torch ops: per window NHWC -> NCHW, F.interpolate to the crop, add_ into the
                           [B, C, H, W] accumulator, divide by the count map, argmax and the library's counting of explicit pairs
                           (segf_confmat_pairs); the peak of the allocator above the inputs while it runs;
  pred_agreement           share of the pixels at which the two predictions agree (they differ only at fp32 near-ties);
  step_ms / kernel_share   engine.evaluate_slide per batch (slicing the windows, one forward of all of them, the kernel; host clock
                           around a synchronised loop) and the kernel's share of it."""
import argparse
import contextlib
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eval-dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--configs', nargs='+', default=[c['name'] for c in CONFIGS], choices=[c['name'] for c in CONFIGS])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_slide.py measures on the GPU'
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    out = {'bench': 'slide_eval', 'eval_dtype': a.eval_dtype, 'cases': []}
    for cfg in (c for c in CONFIGS if c['name'] in a.configs):
        B, H, W, C = cfg['batch'], cfg['H'], cfg['W'], cfg['classes']
        (ch, cw), (sh, sw), origins = engine.slide_windows(H, W, cfg['crop'], cfg['stride'])
        h, w, nwin = ch // 4, cw // 4, len(origins)
        case = dict(cfg, windows=nwin, map=[h, w])
        target = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        target[:, :8] = 255
        mat = torch.zeros((C, C), dtype=torch.int64, device=dev)
        hist, flag = mat.clone(), torch.zeros(1, dtype=torch.int32, device=dev)
        pred = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
            rows = (3 * torch.randn(B * nwin * h * w, C, device=dev, generator=g)).to(dt)
            nbytes = rows.numel() * rows.element_size() + target.numel() * 8 + 2 * C * C * 8
            ms = timeit(lambda: hip.slide_argmax_confmat((rows, h, w), B, C, H, W, (ch, cw), (sh, sw), target, 255, mat, hist, flag), a.iters)
            case[f'kernel_ms_{name}'] = round(ms, 4)
            case[f'kernel_gbs_{name}'] = round(nbytes / ms / 1e6, 1)
            case[f'must_move_mb_{name}'] = round(nbytes / 1e6, 1)
            hip.slide_argmax_confmat((rows, h, w), B, C, H, W, (ch, cw), (sh, sw), None, 255, None, None, None, pred_out=pred)
            maps = rows.view(B, nwin, h, w, C)
            kept = {}

            def restated():
                acc = torch.zeros((B, C, H, W), dtype=torch.float32, device=dev)
                cnt = torch.zeros((1, 1, H, W), dtype=torch.float32, device=dev)
                for k, (y, x) in enumerate(origins):
                    z = F.interpolate(maps[:, k].float().permute(0, 3, 1, 2), size=(ch, cw), mode='bilinear', align_corners=False)
                    acc[:, :, y:y + ch, x:x + cw].add_(z)
                    cnt[:, :, y:y + ch, x:x + cw].add_(1)
                kept['pred'] = acc.div_(cnt).argmax(1)
                hip.confmat_pairs(target.flatten(), kept['pred'].flatten(), C, 255, mat, hist, flag)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            case[f'torch_ms_{name}'] = round(timeit(restated, max(2, a.iters // 5), warm=1), 3)
            case[f'torch_peak_mb_{name}'] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
            case[f'pred_agreement_{name}'] = round((kept['pred'] == pred).float().mean().item(), 6)
            del rows, maps, kept
            torch.cuda.empty_cache()
        # one full sliding-window step: slice the windows, one forward of all of them, the kernel
        model = SegmentationModel('MiT-B0', num_classes=C, seg_head='SegFormerHead').to(dev).eval()
        x = torch.randn(B, 3, H, W, device=dev, generator=g)
        args = types.SimpleNamespace(nb_classes=C, ignore_label=255, eval_dtype=a.eval_dtype)
        kw = dict(crop=cfg['crop'], stride=cfg['stride'])
        with contextlib.redirect_stdout(sys.stderr):                                # the logger's lines: stdout carries the JSON line only
            engine.evaluate_slide(args, model, [(x, target)] * 3, dev, 1000, **kw)  # eager sighting, capture, first replay
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.evaluate_slide(args, model, [(x, target)] * a.steps, dev, 1000, **kw)
            torch.cuda.synchronize()
        step = (time.perf_counter() - t0) * 1e3 / a.steps
        k = case[f'kernel_ms_{a.eval_dtype}']
        case.update(step_ms=round(step, 2), kernel_share=round(k / step, 4))
        out['cases'].append(case)
        del model
        torch.cuda.empty_cache()
    out['fused_not_slower_than_torch'] = all(c[f'kernel_ms_{n}'] <= c[f'torch_ms_{n}'] for c in out['cases'] for n in ('bf16', 'fp32'))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
