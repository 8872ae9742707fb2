"""Time the backward of `norm2 -> mlp.fc1` at the SegFormer-B0 stage-1 / stage-2 shapes (bf16): the launches of today -- segf_gemm (fc1's data
gradient, layout 1), segf_layernorm_bwd_scaled, segf_gemm_dw_db -- against the fused segf_layernorm_linear_bwd, alternating in one process.
Usage: python tools/bench_ln_linear_bwd.py [--out profiles/ln_linear_bwd_fused_ab.jsonl] [--iters 40] [--batches 256 128 16]

One JSON line per shape: per-launch HIP-event times of every form (median, p10, p90 in microseconds), the sum of the separate medians, the
ratio fused / sum, and whether dy, dx and the DropPath-scaled dx came out bit-equal on the same data.  Stage 1 at batch 256 has 2^22 token
rows, where segf_layernorm_bwd_scaled has no scaled output: the step then scales dx with its own segf_scale_rows launch, which is timed as
a fourth member.  The finalizes are deferred on both sides, as in the captured step.  The clocks ramp for the first tens of milliseconds
of load: all forms run alternately for >= 60 ms before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

STAGES = [(128, 128, 32), (64, 64, 64)]          # (H, W, C) of MiT-B0 stages 1 and 2 at 512^2; the hidden width is 4 C


def one_shape(B, H, W, C, iters):
    g = torch.Generator(device='cuda').manual_seed(0)
    rows, N = B * H * W, 4 * C
    rn = lambda *s: torch.randn(*s, generator=g, device='cuda')      # noqa: E731
    x = (rn(rows, C) * 1.5 + 0.3).bfloat16()
    gamma, beta = 1.0 + 0.3 * rn(C), 0.2 * rn(C)
    w1 = (rn(N, C) * 0.2).bfloat16()
    dh, dres = rn(rows, N).bfloat16(), rn(rows, C).bfloat16()
    rscale = (torch.rand(B, generator=g, device='cuda') < 0.9).float() / 0.9
    rpg = H * W
    y, mean, rstd = hip.layernorm_fwd(x, gamma, beta, 1e-5)
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
    f32 = lambda n: torch.empty(max(int(n), 1), dtype=torch.float32, device='cuda')      # noqa: E731
    dy, dx, dxs, dx_f, dxs_f = (torch.empty_like(x) for _ in range(5))
    split = hip.pick_splitk(N, C, rows)
    ws_ln, ws_dw, ws_f = f32(lib.segf_layernorm_bwd_ws(rows, C)), f32(lib.segf_gemm_dw_db_ws(N, C, rows, split)), f32(lib.segf_layernorm_linear_bwd_ws(rows, C, N))
    dw, db1 = torch.empty(N, C, device='cuda'), torch.empty(N, device='cuda')
    P = lambda t: t.data_ptr()      # noqa: E731
    ln_scales = rows < (1 << 22)             # segf_layernorm_bwd_scaled's bound

    def gemm():
        assert lib.segf_gemm(hip.BF16, 1, rows, C, N, P(dh), N, P(w1), C, P(dy), hip.BF16, C, None, None, 0, None, 1, 1, None, st) == 0

    def ln():
        assert lib.segf_layernorm_bwd_scaled(hip.BF16, rows, C, P(x), P(dy), None, P(dres), P(gamma), P(mean), P(rstd), P(dx), None, None, P(ws_ln),
                                             P(rscale) if ln_scales else None, rpg, P(dxs) if ln_scales else None, st) == 0

    def scale():
        assert lib.segf_scale_rows(hip.BF16, P(dx), C, P(dxs), C, P(rscale), rows, C, rpg, st) == 0

    def dwdb():
        assert lib.segf_gemm_dw_db(hip.BF16, N, C, rows, P(dh), N, P(y), C, P(dw), hip.F32, C, split, P(ws_dw), P(db1), st) == 0

    def fused():
        assert lib.segf_layernorm_linear_bwd(hip.BF16, rows, C, N, P(dh), P(w1), P(x), P(y), P(dres), P(gamma), P(mean), P(rstd), P(dx_f), P(rscale), rpg,
                                             P(dxs_f), None, None, None, None, None, P(ws_f), st) == 0

    forms = [('gemm', gemm), ('ln', ln)] + ([] if ln_scales else [('scale_rows', scale)]) + [('dw_db', dwdb), ('fused', fused)]
    # bit-equality once, through the Python wrappers
    dy_ref = hip.gemm(1, dh, w1, rows, C, N)
    ref = hip.layernorm_bwd(x, dy_ref, gamma, mean, rstd, dres=dres, rscale=rscale if ln_scales else None, rows_per_group=rpg)
    dxs_ref = ref[0].scaled if ln_scales else hip.scale_rows(ref[0], rscale, rpg)
    got = hip.layernorm_linear_bwd(dh, w1, x, y, gamma, mean, rstd, dres=dres, rscale=rscale, rows_per_group=rpg, return_dy=True)
    equal = {'dy': torch.equal(got[5], dy_ref), 'dx': torch.equal(got[0], ref[0]), 'dxs': torch.equal(got[0].scaled, dxs_ref)}
    del dy_ref, ref, dxs_ref, got
    t0 = time.perf_counter()
    while True:
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.08:
            break
    times = {name: [] for name, _ in forms}
    evs = []
    for _ in range(iters):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            evs.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in evs:
        times[name].append(e0.elapsed_time(e1) * 1e3)
    kernels = {}
    for name, fn in forms:
        with hip.trace() as t:
            fn()
        kernels[name] = [k.split(' [')[0] for k in t.kernels]
    torch.cuda.synchronize()

    def stat(v):
        v = sorted(v)
        return {'median_us': round(statistics.median(v), 1), 'p10_us': round(v[len(v) // 10], 1), 'p90_us': round(v[(9 * len(v)) // 10], 1)}
    out = {'shape': [B, H, W, C], 'token_rows': rows, 'launches_each': iters}
    for name, _ in forms:
        out[name] = stat(times[name])
    separate = sum(statistics.median(times[name]) for name, _ in forms if name != 'fused')
    out.update({'separate_sum_us': round(separate, 1), 'fused_over_separate': round(statistics.median(times['fused']) / separate, 4),
                'bit_equal': equal, 'supported_by_default': bool(lib.segf_layernorm_linear_bwd_supported(hip.BF16, rows, C, N)),
                'kernels': kernels})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--batches', type=int, nargs='*', default=[256, 128, 16])
    a = ap.parse_args()
    lines = []
    for B in a.batches:
        for (H, W, C) in STAGES:
            lines.append(json.dumps(one_shape(B, H, W, C, a.iters)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
