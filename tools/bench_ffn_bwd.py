"""Time the Mix-FFN backward tail at the SegFormer-B0 stage-1 / stage-2 shapes (bf16): the pair segf_gemm (fc2's data gradient, layout 1)
+ segf_dwconv3x3_gelu_bwd against the fused segf_dwconv3x3_gelu_bwd_fc2, alternating in one process.
Usage: python tools/bench_ffn_bwd.py [--out profiles/ffn_bwd_fused_ab.jsonl] [--iters 40] [--batches 256 128 16 4]
       python tools/bench_ffn_bwd.py --stage34 --batches 256 128 16 --out profiles/ffn_bwd_stage34_ab.jsonl     (stages 3 / 4: W2 fragments in LDS)

One JSON line per shape: per-launch HIP-event times of both forms (median, min, max in microseconds), the ratio of the medians, and
whether all of du / dx / dw / db came out bit-equal.  The clocks ramp for the first tens of milliseconds of load:
both forms run alternately for >= 60 ms before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

STAGES = [(128, 128, 128, 32), (64, 64, 256, 64)]          # (H, W, C_hidden, C_in) of MiT-B0 stages 1 and 2 at 512^2
STAGES34 = [(32, 32, 640, 160), (16, 16, 1024, 256)]       # ... stages 3 and 4 (--stage34: W2 fragments in LDS, profiles/ffn_bwd_stage34_ab.jsonl)


def one_shape(B, H, W, Cc, Cin, iters):
    g = torch.Generator().manual_seed(0)
    M = B * H * W
    f = torch.randn(M, Cc, generator=g).bfloat16().cuda()
    dys = torch.randn(M, Cin, generator=g).bfloat16().cuda()
    w2 = (torch.randn(Cin, Cc, generator=g) * 0.2).bfloat16().cuda()
    w9 = (torch.randn(Cc, 9, generator=g) * 0.3).cuda()
    b = torch.randn(Cc, generator=g).cuda()
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
    dg, du, dx = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    ws = torch.empty(int(lib.segf_dwconv3x3_bwd_ws(B, H, W, Cc)), dtype=torch.float32, device='cuda')
    dw, db = torch.empty(Cc, 9, device='cuda'), torch.empty(Cc, device='cuda')
    P = lambda t: t.data_ptr()      # noqa: E731

    def pair():            # the step's form: deferred finalize (dw == NULL) on both sides
        assert lib.segf_gemm(hip.BF16, 1, M, Cc, Cin, P(dys), Cin, P(w2), Cc, P(dg), hip.BF16, Cc, None, None, 0, None, 1, 1, None, st) == 0
        assert lib.segf_dwconv3x3_gelu_bwd(hip.BF16, B, H, W, Cc, P(f), P(w9), P(b), 1, P(dg), P(du), P(dx), None, None, P(ws), st) == 0

    def fused():
        assert lib.segf_dwconv3x3_gelu_bwd_fc2(hip.BF16, B, H, W, Cc, Cin, P(f), P(w9), P(b), P(dys), Cin, P(w2), P(du), P(dx), None, None, P(ws), st) == 0

    # bit-equality once, through the Python wrappers (direct finalize)
    with hip.policy_override(dw_no_small=1):
        dg_ref = hip.gemm(1, dys, w2, M, Cc, Cin)
        ref = hip.dwconv3x3_gelu_bwd(f, w9, b, dg_ref, B, H, W, Cc, True)
        got = hip.dwconv3x3_gelu_bwd_fc2(f, w9, b, dys, w2, B, H, W, Cc, Cin)
        equal = all(torch.equal(a, c) for a, c in zip(got, ref))
        del dg_ref, ref, got
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
        kernels = {}
        for name, fn in (('pair', pair), ('fused', fused)):
            with hip.trace() as t:
                fn()
            kernels[name] = [k.split(' [')[0] for k in t.kernels]
    torch.cuda.synchronize()
    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {'median_us': round(statistics.median(v), 1), 'p10_us': round(q[0], 1), 'p90_us': round(q[-1], 1), 'min_us': round(min(v), 1),
                'max_us': round(max(v), 1)}
    return {'shape': [B, H, W, Cc, Cin], 'token_rows': M, 'launches_each': iters, 'pair': stat(times['pair']), 'fused': stat(times['fused']),
            'fused_over_pair': round(statistics.median(times['fused']) / statistics.median(times['pair']), 4), 'bit_equal': equal,
            'supported_by_default': bool(lib.segf_dwconv3x3_gelu_bwd_fc2_supported(hip.BF16, B, H, W, Cc, Cin)
                                         or lib.segf_dwconv3x3_gelu_bwd_fc2_lds_supported(hip.BF16, B, H, W, Cc, Cin)),
            'pair_gemm_kernel': kernels['pair'][0], 'fused_kernel': kernels['fused'][0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--batches', type=int, nargs='*', default=[256, 128, 16, 4])
    ap.add_argument('--stage34', action='store_true', help='the stage-3 / stage-4 shapes instead of stages 1 / 2')
    a = ap.parse_args()
    lines = []
    for B in a.batches:
        for (H, W, Cc, Cin) in (STAGES34 if a.stage34 else STAGES):
            lines.append(json.dumps(one_shape(B, H, W, Cc, Cin, a.iters)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
