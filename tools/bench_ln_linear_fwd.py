"""Time `LayerNorm -> thin Linear` at the SegFormer-B0 stage-1 / stage-2 shapes (bf16), the separate launches against the one-pass forms,
alternating in one process.
Usage: python tools/bench_ln_linear_fwd.py [--out profiles/ln_linear_fwd_fused_ab.jsonl] [--iters 40] [--batches 256 128 16]

One JSON line per (shape, part):
  fwd_fc1   segf_layernorm_fwd + segf_gemm (layout 0, N = 4 C)                          against segf_layernorm_linear_fwd
  fwd_q     segf_layernorm_fwd_patch (y and its patch-major copy) + segf_gemm (N = C)   against segf_layernorm_linear_fwd (patch-major copy only)
  bwd_q     segf_gemm (layout 1) + segf_gemm_dw_db + segf_layernorm_bwd_patch           against segf_layernorm_linear_bwd_ex (N = C, y rebuilt)
  bwd_fc1   segf_layernorm_linear_bwd reading the stored y                              against segf_layernorm_linear_bwd_ex rebuilding it
with the per-launch HIP-event times of every member (median, p10, p90 in microseconds), the sum of the separate medians, the fused median,
the ratio fused / sum and the bit-equality of the data tensors on the same data.  The finalizes are deferred on both sides, as in the
captured step; the DropPath-scaled output is asked for where segf_layernorm_bwd_scaled has it (below 2^22 rows).  The clocks ramp for the
first tens of milliseconds of load: all forms run alternately for >= 60 ms before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_factory_amd import hip   # noqa: E402

STAGES = [(128, 128, 32, 8), (64, 64, 64, 4)]          # (H, W, C, sr) of MiT-B0 stages 1 and 2 at 512^2
EPS = 1e-5


def time_forms(forms, iters):
    t0 = time.perf_counter()
    while True:
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.08:
            break
    times, evs = {name: [] for name, _ in forms}, []
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
    out = {name: stat(times[name]) for name, _ in forms}
    separate = sum(statistics.median(times[name]) for name, _ in forms if name != 'fused')
    fused = statistics.median(times['fused'])
    out.update({'separate_sum_us': round(separate, 1), 'fused_us': round(fused, 1), 'fused_over_separate': round(fused / separate, 4), 'kernels': kernels})
    return out


def one_shape(B, H, W, C, sr, iters):
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = B * H * W
    lw, ls = W.bit_length() - 1, sr.bit_length() - 1
    rn = lambda *s: torch.randn(*s, generator=g, device='cuda')      # noqa: E731
    x = (rn(rows, C) * 1.5 + 0.3).bfloat16()
    gamma, beta = 1.0 + 0.3 * rn(C), 0.2 * rn(C)
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
    f32 = lambda n: torch.empty(max(int(n), 1), dtype=torch.float32, device='cuda')      # noqa: E731
    P = lambda t: t.data_ptr()      # noqa: E731
    mean, rstd, mean_f, rstd_f = f32(rows), f32(rows), f32(rows), f32(rows)
    y, col, col_f = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    base = {'shape': [B, H, W, C], 'token_rows': rows, 'launches_each': iters}
    lines = []
    # ---- forward, both widths
    for part, N, patch in (('fwd_fc1', 4 * C, False), ('fwd_q', C, True)):
        w, bias = (rn(N, C) * 0.2).bfloat16(), 0.5 * rn(N)
        out, out_f = torch.empty(rows, N, dtype=torch.bfloat16, device='cuda'), torch.empty(rows, N, dtype=torch.bfloat16, device='cuda')

        def ln(patch=patch):
            assert lib.segf_layernorm_fwd_patch(hip.BF16, rows, C, P(x), P(gamma), P(beta), EPS, P(y), P(mean), P(rstd), P(col) if patch else None, lw, ls, st) == 0

        def gemm(N=N, w=w, bias=bias, out=out):
            assert lib.segf_gemm(hip.BF16, 0, rows, N, C, P(y), C, P(w), C, P(out), hip.BF16, N, P(bias), None, 0, None, 1, 1, None, st) == 0

        def fused(N=N, w=w, bias=bias, out_f=out_f, patch=patch):
            assert lib.segf_layernorm_linear_fwd(hip.BF16, rows, C, N, P(x), P(gamma), P(beta), EPS, P(w), P(bias), P(out_f), P(mean_f), P(rstd_f), None,
                                                 P(col_f) if patch else None, lw, ls, st) == 0
        forms = [('ln', ln), ('gemm', gemm), ('fused', fused)]
        ln(); gemm(); fused()
        torch.cuda.synchronize()
        equal = {'out': torch.equal(out_f, out), 'mean': torch.equal(mean_f, mean), 'rstd': torch.equal(rstd_f, rstd)}
        if patch:
            equal['col'] = torch.equal(col_f, col)
        r = dict(base, part=part, N=N, **time_forms(forms, iters), bit_equal=equal,
                 supported_by_default=bool(lib.segf_layernorm_linear_fwd_supported(hip.BF16, rows, C, N)))
        lines.append(r)
        del w, bias, out, out_f
    # ---- backward of norm1 -> q against its three launches; of norm2 -> fc1 with the stored against the rebuilt y
    hip.lib().segf_layernorm_fwd_patch(hip.BF16, rows, C, P(x), P(gamma), P(beta), EPS, P(y), P(mean), P(rstd), None, 0, 0, st)
    dres, dcol = rn(rows, C).bfloat16(), rn(rows, C).bfloat16()
    rscale = (torch.rand(B, generator=g, device='cuda') < 0.9).float() / 0.9
    rpg = H * W
    scales = rows < (1 << 22)                # segf_layernorm_bwd_scaled's bound: the one-pass forms get the same request
    dy, dx, dxs, dx_f, dxs_f = (torch.empty_like(x) for _ in range(5))
    rs_p, dxs_p, dxsf_p = (P(rscale), P(dxs), P(dxs_f)) if scales else (None, None, None)
    for part, N in (('bwd_q', C), ('bwd_fc1', 4 * C)):
        w = (rn(N, C) * 0.2).bfloat16()
        dh = rn(rows, N).bfloat16()
        ws_f = f32(lib.segf_layernorm_linear_bwd_ws(rows, C, N))
        if part == 'bwd_q':
            split = hip.pick_splitk(N, C, rows)
            ws_ln, ws_dw = f32(lib.segf_layernorm_bwd_ws(rows, C)), f32(lib.segf_gemm_dw_db_ws(N, C, rows, split))
            dw, db1 = torch.empty(N, C, device='cuda'), torch.empty(N, device='cuda')

            def gemm():
                assert lib.segf_gemm(hip.BF16, 1, rows, C, N, P(dh), N, P(w), C, P(dy), hip.BF16, C, None, None, 0, None, 1, 1, None, st) == 0

            def dwdb():
                assert lib.segf_gemm_dw_db(hip.BF16, N, C, rows, P(dh), N, P(y), C, P(dw), hip.F32, C, split, P(ws_dw), P(db1), st) == 0

            def ln():
                assert lib.segf_layernorm_bwd_patch(hip.BF16, rows, C, P(x), P(dy), P(dcol), P(dres), P(gamma), P(mean), P(rstd), P(dx), None, None, P(ws_ln),
                                                    rs_p, rpg, dxs_p, lw, ls, st) == 0

            def fused():
                assert lib.segf_layernorm_linear_bwd_ex(hip.BF16, rows, C, N, P(dh), P(w), P(x), None, P(beta), P(dcol), lw, ls, P(dres), P(gamma), P(mean),
                                                        P(rstd), P(dx_f), rs_p, rpg, dxsf_p, None, None, None, None, None, P(ws_f), st) == 0
            forms = [('gemm', gemm), ('dw_db', dwdb), ('ln', ln), ('fused', fused)]
        else:
            def stored():
                assert lib.segf_layernorm_linear_bwd(hip.BF16, rows, C, N, P(dh), P(w), P(x), P(y), P(dres), P(gamma), P(mean), P(rstd), P(dx), rs_p, rpg,
                                                     dxs_p, None, None, None, None, None, P(ws_f), st) == 0

            def fused():
                assert lib.segf_layernorm_linear_bwd_ex(hip.BF16, rows, C, N, P(dh), P(w), P(x), None, P(beta), None, -1, 0, P(dres), P(gamma), P(mean),
                                                        P(rstd), P(dx_f), rs_p, rpg, dxsf_p, None, None, None, None, None, P(ws_f), st) == 0
            forms = [('stored_y', stored), ('fused', fused)]
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        equal = {'dx': torch.equal(dx_f, dx)}
        if scales:
            equal['dxs'] = torch.equal(dxs_f, dxs)
        r = dict(base, part=part, N=N, **time_forms(forms, iters), bit_equal=equal,
                 supported_by_default=bool(lib.segf_layernorm_linear_bwd_ex_supported(hip.BF16, rows, C, N)))
        lines.append(r)
        del w, dh, ws_f
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--batches', type=int, nargs='*', default=[256, 128, 16])
    a = ap.parse_args()
    lines = []
    for B in a.batches:
        for (H, W, C, sr) in STAGES:
            for r in one_shape(B, H, W, C, sr, a.iters):
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
