"""Time the head-dim-32 attention kernels at the four SegFormer-B0 stage shapes of the 512^2 configs (bf16, 256 keys): the default
backward arithmetic (fma + exp2, -D inside the dP products) against the round-2 arithmetic (policy attn32_classic), alternating in
one process; the forward, which has one form, is timed beside it under both settings as a control.
Usage: python tools/bench_attn32.py [--out FILE (default profiles/attn32_lean_ab.jsonl)] [--iters 40] [--batches 256 4]

One JSON line per shape: per-launch HIP-event times of the forward and of the backward (fused kernel + attn_dkv_reduce) under both
policies (median, p10, p90 in microseconds) and the ratio of the medians.  The clocks ramp for the first tens of milliseconds of
load: both forms run alternately for >= 60 ms before anything is timed.  The backward of each policy runs on the
o / lse of that policy's own forward."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

HD = 32
STAGES = [(1, 16384), (2, 4096), (5, 1024), (8, 256)]          # (heads, N) of MiT-B0 stages 1-4 at 512^2; Nkv = 256 in all four
NKV = 256


def one_shape(B, heads, N, iters):
    g = torch.Generator().manual_seed(0)
    C = heads * HD
    q, do = (torch.randn(B * N, C, generator=g).bfloat16().cuda() for _ in range(2))
    kv = torch.randn(B * NKV, 2 * C, generator=g).bfloat16().cuda()
    k, v = kv[:, :C], kv[:, C:]
    dkv = torch.empty_like(kv)
    scale = HD ** -0.5
    state, kernels = {}, {}
    for name, classic in (('classic', 1), ('new', 0)):
        with hip.policy_override(attn32_classic=classic):
            with hip.trace() as t:
                o, lse = hip.attention_fwd(q, k, v, B, heads, N, NKV, HD, scale)
                hip.attention_bwd(q, k, v, o, do, lse, B, heads, N, NKV, HD, scale, dkv[:, :C], dkv[:, C:])
            kernels[name] = [x.split(' [')[0] for x in t.kernels]
            state[name] = (classic, o, lse)

    def fwd(name):
        with hip.policy_override(attn32_classic=state[name][0]):
            hip.attention_fwd(q, k, v, B, heads, N, NKV, HD, scale)

    def bwd(name):
        classic, o, lse = state[name]
        with hip.policy_override(attn32_classic=classic):
            hip.attention_bwd(q, k, v, o, do, lse, B, heads, N, NKV, HD, scale, dkv[:, :C], dkv[:, C:])

    t0 = time.perf_counter()
    while True:
        for name in ('classic', 'new'):
            fwd(name); bwd(name)
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.08:
            break
    evs = []
    for _ in range(iters):
        for what, fn in (('fwd', fwd), ('bwd', bwd)):
            for name in ('classic', 'new'):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(name); e1.record()
                evs.append((what, name, e0, e1))
    torch.cuda.synchronize()
    times = {}
    for what, name, e0, e1 in evs:
        times.setdefault((what, name), []).append(e0.elapsed_time(e1) * 1e3)

    def stat(v):
        qs = statistics.quantiles(v, n=10)
        return {'median_us': round(statistics.median(v), 1), 'p10_us': round(qs[0], 1), 'p90_us': round(qs[-1], 1)}

    out = {'shape': [B, heads, N, NKV, HD], 'launches_each': iters, 'kernels': kernels}
    for what in ('fwd', 'bwd'):
        out[what] = {name: stat(times[(what, name)]) for name in ('classic', 'new')}
        out[what + '_new_over_classic'] = round(statistics.median(times[(what, 'new')]) / statistics.median(times[(what, 'classic')]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'attn32_lean_ab.jsonl'))
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--batches', type=int, nargs='*', default=[256, 4])
    a = ap.parse_args()
    lines = []
    for B in a.batches:
        for heads, N in STAGES:
            lines.append(json.dumps(one_shape(B, heads, N, a.iters)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
