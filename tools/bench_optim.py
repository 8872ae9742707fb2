#!/usr/bin/env python3
"""Same-process A/B of the fused optimizer step kernels over the real flat layouts of BASELINE cfg2 (MiT-B0 + the 768-wide SegFormerHead at 150
classes, 6.2 M parameters) and cfg5 (convnextv2_large + UPerHead, 235 M): segf_agc_adamw next to every rule of segf_flat_optim_step, with the
unit-wise AGC pass on and off.

The layout (offsets, unit tables, weight-decay flags) is what FusedAGCAdamW builds for the model; every rule is launched on those
tables with its own state buffers.  Timing: HIP events around single launches, the rules interleaved round-robin (launch k of every
rule before launch k + 1 of any), `--warmup` untimed rounds, `--launches` timed ones (>= 20).  Per rule: median, 10th..90th
percentile spread, min, max, and GB/s against the bytes the rule must move per parameter (fp32: read p, g and each state buffer,
write p and each state buffer: 12 B without state, 20 B with one buffer, 28 B with two; the AGC pass re-reads p and g, which is NOT
counted -- the AGC-on figures are lower bounds of the traffic).  One JSON line per (config, agc) with every rule, and a verdict per
rule: its median may exceed segf_agc_adamw's by at most the spread observed for segf_agc_adamw in the same run.

python tools/bench_optim.py [--configs cfg2 cfg5] [--launches 40] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'cfg2': ('MiT-B0', 'SegFormerHead', 150), 'cfg5': ('convnextv2_large', 'UPerHead', 171)}
LR, WD, EPS = 1e-4, 0.025, 1e-8


def _rules(hip):
    """[(name, bytes per parameter, state buffers, launcher(o, s0, s1, agc))]"""
    def adamw(o, s0, s1, agc, t=[0]):
        t[0] += 1
        hip.agc_adamw(o._flat, o._grad, s0, s1, o._off, o._len, o._flags, LR, 0.9, 0.999, EPS, WD, t[0], agc, unit_step=o._ustep)

    def rule(name, **kw):
        def go(o, s0, s1, agc):
            hip.flat_optim_step(name, o._flat, o._grad, s0, s1, o._off, o._len, o._flags, o._ustep, LR, WD, clip_factor=agc, **kw)
        return go
    return [('agc_adamw', 28, 2, adamw),
            ('sgd_nesterov', 20, 1, rule('sgd', h0=0.9, nesterov=True)),
            ('sgd_momentum', 20, 1, rule('sgd', h0=0.9)),
            ('sgd_plain', 12, 0, rule('sgd', h0=0.0)),
            ('adam', 28, 2, rule('adam', h0=0.9, h1=0.999, eps=EPS)),
            ('rmsprop_momentum', 28, 2, rule('rmsprop', h0=0.9, h1=0.9, eps=EPS)),
            ('rmsprop_plain', 20, 1, rule('rmsprop', h0=0.9, h1=0.0, eps=EPS))]


def run(cfg, launches, warmup):
    from segmentation_factory_amd import SegmentationModel, hip
    from segmentation_factory_amd.optim import FusedAGCAdamW, param_groups_weight_decay
    backbone, head, nc = CONFIGS[cfg]
    model = SegmentationModel(backbone, num_classes=nc, seg_head=head).cuda()
    opt = FusedAGCAdamW(param_groups_weight_decay(model, WD), lr=LR)
    opt.ensure_built(order=list(model.parameters()))
    n = sum(p.numel() for p in opt._params)
    g = torch.Generator(device='cuda').manual_seed(1)
    opt._grad.copy_(torch.randn(opt._grad.numel(), generator=g, device='cuda') * 1e-2)
    rules = _rules(hip)
    state = {name: [torch.zeros_like(opt._flat) for _ in range(ns)] + [None] * (2 - ns) for name, _, ns, _ in rules}    # each rule its own
    out = []
    for agc in (0.0, 0.02):
        times = {name: [] for name, _, _, _ in rules}
        for k in range(warmup + launches):
            for name, _, _, go in rules:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                go(opt, state[name][0], state[name][1], agc)
                e1.record()
                e1.synchronize()
                if k >= warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)          # us
        base = np.asarray(times['agc_adamw'])
        base_med, base_spread = float(np.median(base)), float(np.percentile(base, 90) - np.percentile(base, 10))
        res = {'config': cfg, 'parameters': n, 'units': int(opt._len.numel()), 'agc': agc > 0, 'launches': launches, 'warmup': warmup,
               'agc_adamw_spread_us': round(base_spread, 2), 'rules': {}}
        for name, bpp, _, _ in rules:
            t = np.asarray(times[name])
            med = float(np.median(t))
            res['rules'][name] = {'median_us': round(med, 2), 'p10_us': round(float(np.percentile(t, 10)), 2),
                                  'p90_us': round(float(np.percentile(t, 90)), 2), 'min_us': round(float(t.min()), 2),
                                  'max_us': round(float(t.max()), 2), 'bytes_per_param': bpp,
                                  'GBps': round(bpp * n / (med * 1e-6) / 1e9, 1),
                                  'within_adamw_plus_spread': bool(med <= base_med + base_spread)}
        assert torch.isfinite(opt._flat).all(), 'the parameters left the finite range during the timing loop'
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--configs', nargs='+', default=['cfg2', 'cfg5'], choices=sorted(CONFIGS))
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args()
    if args.launches < 20:
        ap.error('--launches must be at least 20')
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_optim.py times kernels on the GPU: no device found')
    lines = [r for cfg in args.configs for r in run(cfg, args.launches, args.warmup)]
    if args.out:
        with open(args.out, 'w') as fh:
            fh.writelines(json.dumps(r) + '\n' for r in lines)


if __name__ == '__main__':
    main()
