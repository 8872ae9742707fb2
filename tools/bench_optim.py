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

--groups: the leg of the per-group learning rates instead.  Every rule is timed in its scalar form and in its group form
(segf_agc_adamw_groups / segf_flat_optim_step_groups) with 4 and with 108 groups (--head-lr-mult; --layer-decay on MiT-B5), the units
dealt to the groups parameter by parameter, all on the same flat buffers, and -- with --parent-lib, another build of the library,
loaded into the same process -- next to THAT build's scalar kernel, which is the baseline: never the new build against itself.  The
variants are interleaved round-robin with the order rotated from round to round (what a launch finds in the caches depends on the
launch before it), in three runs of --launches launches each.  Margin: the spread of the baseline's three run medians,
plus that much again; a variant passes when its median over the runs is within baseline median + margin.  Bytes per parameter as above;
the group forms read one more byte per UNIT (a row), listed as bytes_per_unit_extra.

python tools/bench_optim.py --groups --configs cfg2 b2 --parent-lib /path/to/parent/libsegfac_hip.so
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'cfg2': ('MiT-B0', 'SegFormerHead', 150), 'cfg5': ('convnextv2_large', 'UPerHead', 171), 'b2': ('MiT-B2', 'SegFormerHead', 150)}
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


def _group_rules(hip):
    """[(name, bytes per parameter, state buffers, scalar launcher(o, s0, s1, agc), group launcher(o, s0, s1, agc, unit_group, lrs, wds))]"""
    def adamw_groups(o, s0, s1, agc, ug, lrs, wds, t=[0]):
        t[0] += 1
        hip.agc_adamw_groups(o._flat, o._grad, s0, s1, o._off, o._len, o._flags, ug, lrs, wds, 0.9, 0.999, EPS, t[0], agc, unit_step=o._ustep)

    def rule(name, **kw):
        def go(o, s0, s1, agc, ug, lrs, wds):
            hip.flat_optim_step_groups(name, o._flat, o._grad, s0, s1, o._off, o._len, o._flags, o._ustep, ug, lrs, wds, clip_factor=agc, **kw)
        return go
    groups = {'agc_adamw': adamw_groups, 'sgd_nesterov': rule('sgd', h0=0.9, nesterov=True), 'sgd_momentum': rule('sgd', h0=0.9),
              'sgd_plain': rule('sgd', h0=0.0), 'adam': rule('adam', h0=0.9, h1=0.999, eps=EPS),
              'rmsprop_momentum': rule('rmsprop', h0=0.9, h1=0.9, eps=EPS), 'rmsprop_plain': rule('rmsprop', h0=0.9, h1=0.0, eps=EPS)}
    return [(name, bpp, ns, go, groups[name]) for name, bpp, ns, go in _rules(hip)]


class _use_lib:
    """Route hip.lib() to another loaded build for the calls inside the block (the scalar entry points only)."""

    def __init__(self, hip, other):
        self.hip, self.other = hip, other

    def __enter__(self):
        self.mine = self.hip.lib()
        self.hip._lib = self.other

    def __exit__(self, *exc):
        self.hip._lib = self.mine
        return False


def _load_parent(hip, path):
    lib = C.CDLL(path)
    for name in ('segf_agc_adamw', 'segf_flat_optim_step'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip._DECLS[name]
    return lib


def run_groups(cfg, launches, warmup, parent_path, runs=3):
    from segmentation_factory_amd import SegmentationModel, hip
    from segmentation_factory_amd.optim import FusedAGCAdamW, param_groups_weight_decay
    backbone, head, nc = CONFIGS[cfg]
    model = SegmentationModel(backbone, num_classes=nc, seg_head=head).cuda()
    opt = FusedAGCAdamW(param_groups_weight_decay(model, WD), lr=LR)
    opt.ensure_built(order=list(model.parameters()))
    n, units = sum(p.numel() for p in opt._params), int(opt._len.numel())
    g = torch.Generator(device='cuda').manual_seed(1)
    opt._grad.copy_(torch.randn(opt._grad.numel(), generator=g, device='cuda') * 1e-2)
    parent = _load_parent(hip, parent_path) if parent_path else None
    tables = {}
    for ng in (4, 108):          # parameter k -> group k mod ng; every group the same lr, the decays {0, WD} by the unit's own flag
        ug = torch.zeros(units, dtype=torch.uint8)
        flags = opt._flags.cpu()
        for k, (lo, hi) in enumerate(opt._unit_range):
            ug[lo:hi] = (2 * (k % (ng // 2)) + int(flags[lo])) % ng
        tables[ng] = (ug.cuda(), [LR] * ng, [WD if gi % 2 else 0.0 for gi in range(ng)])
    rules = _group_rules(hip)
    variants = (['parent_scalar'] if parent else []) + ['scalar', 'groups4', 'groups108']
    base = variants[0]
    state = {(name, v): [torch.zeros_like(opt._flat) for _ in range(ns)] + [None] * (2 - ns) for name, _, ns, _, _ in rules for v in variants}
    out = []
    for agc in (0.0, 0.02):
        times = {(name, v): [[] for _ in range(runs)] for name, _, _, _, _ in rules for v in variants}
        for r in range(runs):
            for k in range(warmup + launches):
                for name, _, _, scalar, grouped in rules:
                    for i in range(len(variants)):
                        v = variants[(i + k) % len(variants)]      # rotate: every variant follows every other equally often (cache state)
                        s0, s1 = state[(name, v)]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        if v == 'parent_scalar':
                            with _use_lib(hip, parent):
                                scalar(opt, s0, s1, agc)
                        elif v == 'scalar':
                            scalar(opt, s0, s1, agc)
                        else:
                            grouped(opt, s0, s1, agc, *tables[int(v[6:])])
                        e1.record()
                        e1.synchronize()
                        if k >= warmup:
                            times[(name, v)][r].append(e0.elapsed_time(e1) * 1e3)          # us
        res = {'leg': 'groups', 'config': cfg, 'parameters': n, 'units': units, 'agc': agc > 0, 'launches': launches, 'warmup': warmup,
               'runs': runs, 'baseline': base, 'bytes_per_unit_extra': 1, 'rules': {}}
        for name, bpp, _, _, _ in rules:
            meds = {v: [float(np.median(t)) for t in times[(name, v)]] for v in variants}
            spread = max(meds[base]) - min(meds[base])
            base_med = float(np.median(np.concatenate(times[(name, base)])))
            row = {'baseline_run_medians_us': [round(m, 2) for m in meds[base]], 'baseline_spread_us': round(spread, 2),
                   'margin_us': round(2 * spread, 2), 'bytes_per_param': bpp}
            for v in variants:
                med = float(np.median(np.concatenate(times[(name, v)])))
                row[v] = {'median_us': round(med, 2), 'run_medians_us': [round(m, 2) for m in meds[v]],
                          'GBps': round(bpp * n / (med * 1e-6) / 1e9, 1), 'within_margin': bool(med <= base_med + 2 * spread)}
            res['rules'][name] = row
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
    ap.add_argument('--groups', action='store_true', help='the per-group learning-rate leg: scalar against group forms (4 and 108 groups)')
    ap.add_argument('--parent-lib', default=None, help='--groups: another build of libsegfac_hip.so whose scalar kernels are the baseline')
    args = ap.parse_args()
    if args.launches < 20:
        ap.error('--launches must be at least 20')
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_optim.py times kernels on the GPU: no device found')
    if args.groups:
        lines = [r for cfg in args.configs for r in run_groups(cfg, args.launches, args.warmup, args.parent_lib)]
    else:
        lines = [r for cfg in args.configs for r in run(cfg, args.launches, args.warmup)]
    if args.out:
        with open(args.out, 'w') as fh:
            fh.writelines(json.dumps(r) + '\n' for r in lines)


if __name__ == '__main__':
    main()
