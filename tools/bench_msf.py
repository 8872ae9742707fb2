#!/usr/bin/env python3
"""Multi-scale + flip evaluation: the fused kernel (segf_msf_argmax_confmat) against the bytes it must move, against the unfused
torch restatement on the same GPU, and as a share of one full MSF step of MiT-B0 + SegFormerHead.  One process, one JSON line.

    python tools/bench_msf.py [--batch 8] [--size 512] [--classes 19 150] [--eval-dtype fp32]

Per class count: the 12 maps of the default scales (0.5 ... 1.75, stride-4 head outputs) with flip;
  kernel_ms / kernel_gbs   device-event time of the kernel alone and its rate over the bytes it MUST read and write (every map once,
                           the labels once, the two count matrices), for bf16 and fp32 maps;
  torch_ms                 the same result from torch ops: per map NHWC -> NCHW (+ flip), F.interpolate, softmax, add; then argmax
                           and the library's counting of explicit pairs (segf_confmat_pairs);
  step_ms / kernel_share   engine.evaluate_msf per batch (resize of the input, 12 forwards, the kernel; host clock around a
                           synchronised loop), the kernel's share of it, and the share of the input resizes + flips alone."""
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
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--classes', type=int, nargs='+', default=[19, 150])
    ap.add_argument('--eval-dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_msf.py measures on the GPU'
    B, H, dev = a.batch, a.size, 'cuda'
    sizes = engine.msf_sizes(H, H, engine.MSF_SCALES)
    g = torch.Generator(device=dev).manual_seed(0)
    out = {'bench': 'msf_eval', 'batch': B, 'size': H, 'scales': list(engine.MSF_SCALES), 'flip': True, 'maps': 2 * len(sizes),
           'eval_dtype': a.eval_dtype, 'cases': []}
    for C in a.classes:
        case = {'classes': C}
        target = torch.randint(0, C, (B, H, H), device=dev, generator=g)
        target[:, :8] = 255
        mat = torch.zeros((C, C), dtype=torch.int64, device=dev)
        hist, flag = mat.clone(), torch.zeros(1, dtype=torch.int32, device=dev)
        flips = [k & 1 for k in range(2 * len(sizes))]
        for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
            maps = [(3 * torch.randn(B * (sh // 4) * (sw // 4), C, device=dev, generator=g)).to(dt) for sh, sw in sizes for _ in (0, 1)]
            rows = [(m, sh // 4, sw // 4) for m, (sh, sw) in zip(maps, [s for s in sizes for _ in (0, 1)])]
            nbytes = sum(m.numel() * m.element_size() for m in maps) + target.numel() * 8 + 2 * C * C * 8
            ms = timeit(lambda: hip.msf_argmax_confmat(rows, flips, B, C, H, H, target, 255, mat, hist, flag), a.iters)
            case[f'kernel_ms_{name}'] = round(ms, 4)
            case[f'kernel_gbs_{name}'] = round(nbytes / ms / 1e6, 1)
            case[f'must_move_mb_{name}'] = round(nbytes / 1e6, 1)

            def restated():
                S = None
                for (m, h, w), f in zip(rows, flips):
                    z = m.view(B, h, w, C).float()
                    if f:
                        z = z.flip(2)
                    p = F.interpolate(z.permute(0, 3, 1, 2), size=(H, H), mode='bilinear', align_corners=False).softmax(1)
                    S = p if S is None else S.add_(p)
                hip.confmat_pairs(target.flatten(), S.argmax(1).flatten(), C, 255, mat, hist, flag)
            case[f'torch_ms_{name}'] = round(timeit(restated, max(2, a.iters // 4), warm=1), 3)
            del maps, rows
            torch.cuda.empty_cache()
        # one full MSF step: resize, 12 forwards, the kernel
        model = SegmentationModel('MiT-B0', num_classes=C, seg_head='SegFormerHead').to(dev).eval()
        x = torch.randn(B, 3, H, H, device=dev, generator=g)
        args = types.SimpleNamespace(nb_classes=C, ignore_label=255, eval_dtype=a.eval_dtype)
        with contextlib.redirect_stdout(sys.stderr):                                # the logger's lines: stdout carries the JSON line only
            engine.evaluate_msf(args, model, [(x, target)] * 2, dev, 1000)          # eager sighting, captures, first replays
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.evaluate_msf(args, model, [(x, target)] * a.steps, dev, 1000)
            torch.cuda.synchronize()
        step = (time.perf_counter() - t0) * 1e3 / a.steps

        def resizes():
            for s in sizes:
                xs = x if s == (H, H) else F.interpolate(x, size=s, mode='bilinear', align_corners=False)
                xs.flip(3)
        rs = timeit(resizes, a.iters)
        k = case[f'kernel_ms_{a.eval_dtype}']
        case.update(step_ms=round(step, 2), kernel_share=round(k / step, 4), input_resize_flip_ms=round(rs, 3),
                    input_resize_flip_share=round(rs / step, 4))
        out['cases'].append(case)
        del model
        torch.cuda.empty_cache()
    out['fused_not_slower_than_torch'] = all(c[f'kernel_ms_{n}'] <= c[f'torch_ms_{n}'] for c in out['cases'] for n in ('bf16', 'fp32'))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
