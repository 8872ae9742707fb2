"""Time the classifier's bias gradient riding on pass 1 of the fused BatchNorm backward (bf16, cfg2's head: C = 768, K = 160, 128 x 128
maps): the pair segf_colsum + segf_bn_cls_bwd_full against segf_bn_cls_bwd_full_db, alternating in one process.
Usage: python tools/bench_head_db.py [--out profiles/head_db_ride_ab.jsonl] [--iters 40] [--batches 256 128]

One JSON line per shape: per-call HIP-event times of both forms (median, p10, p90 in microseconds), the ratio of the medians, whether
dx / dgamma / dbeta / dG / dwcls came out bit-equal, and the error of both bias gradients against the float64 column sum.  Both forms run
alternately for >= 60 ms before anything is timed (the clocks ramp for the first tens of milliseconds of load)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402


def one_shape(B, rps, C, K, iters):
    g = torch.Generator().manual_seed(0)
    M = B * rps
    x = torch.empty(M, C, dtype=torch.bfloat16, device='cuda').normal_(0.3, 1.5)
    dy = torch.empty(M, K, dtype=torch.bfloat16, device='cuda').normal_(0, 1e-3)
    w = (torch.randn(K, C, generator=g) / C ** 0.5).bfloat16().cuda()
    gam, bet = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    mean = x.float().mean(0)
    rstd = 1.0 / torch.sqrt(x.float().var(0, unbiased=False) + 1e-5)
    drop = ((torch.rand(B, C, generator=g) > 0.1).float() / 0.9).cuda()
    x1 = torch.empty(M, 32, dtype=torch.bfloat16, device='cuda').normal_(0, 0.7)
    args = (dy, w, x, mean, rstd, gam, bet, 1, drop, rps, False)

    def pair():
        db = hip.colsum(dy)
        return hip.bn_cls_bwd_full(*args, x1=x1) + (db,)

    def fused():
        return hip.bn_cls_bwd_full_db(*args, x1=x1)

    with hip.policy_override(head_db_ride=2):
        ref, got = pair(), fused()
        equal = all(torch.equal(a, b) for a, b in zip(got[:5], ref[:5]))
        want = dy.double().sum(0)
        err = {'pair': (ref[5].double() - want).abs().max().item(), 'fused': (got[5].double() - want).abs().max().item()}
        del ref, got
        t0 = time.perf_counter()
        while True:
            pair(); fused()
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > 0.08:
                break
        times = {'pair': [], 'fused': []}
        evs = []
        for _ in range(iters):
            for name, fn in (('pair', pair), ('fused', fused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                evs.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in evs:
            times[name].append(e0.elapsed_time(e1) * 1e3)

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {'median_us': round(statistics.median(v), 1), 'p10_us': round(q[0], 1), 'p90_us': round(q[-1], 1)}
    return {'shape': [B, rps, C, K], 'token_rows': M, 'calls_each': iters, 'pair': stat(times['pair']), 'fused': stat(times['fused']),
            'fused_over_pair': round(statistics.median(times['fused']) / statistics.median(times['pair']), 4), 'others_bit_equal': equal,
            'db_max_abs_err_vs_float64': err,
            'supported_by_default': bool(hip.lib().segf_bn_cls_bwd_full_db_supported(hip.BF16, M, C, K, rps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--batches', type=int, nargs='*', default=[256, 128])
    a = ap.parse_args()
    lines = []
    for B in a.batches:
        lines.append(json.dumps(one_shape(B, 128 * 128, 768, 160, a.iters)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
