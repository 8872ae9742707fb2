"""Times one batch of the training input path with the class-balanced crop choice (segf_input_crop_select + segf_input_train,
segf_input_train_scaled_select) beside the SAME batch with the feature off (segf_input_train, segf_input_train_scaled) in the same
process, and writes profiles/input_balanced_crop.md.

    python tools/bench_input_balanced.py [--step-ms X] [--out profiles/input_balanced_crop.md]

512 x 512 crops of 2048 x 1024 (w x h) sources, batch 256 and batch 4, tries = 10 (K = 11 candidate windows), full jitter, on the
unscaled stack and on the scaled one at 0.5 / 1.0 / 2.0, for three label sets:
  (a) 64 x 64 blocks of 19 classes: window 0 passes, every label of the window is read once;
  (b) one class everywhere: all ten tested windows fail, and every lane of every wave hits the same counter;
  (c) one class in the left three quarters, blocks in the right quarter, the first four windows inside the one-class part and the
      later ones flush with the right edge: the walk passes at the fifth window.
Each timing is the median of ROUNDS rounds of ITERS calls, the two paths alternating; device events around the calls, records packed
beforehand (the scaled entry points upload their records and wait for the stream inside the call, on and off alike).  Feature off =
the plain entry point on the first window of the same draws: the parent commit's path, unchanged by construction.  --step-ms:
`ms_per_step` of `bench.py --gpus 1` (batch 256, 512 x 512) from the same session, to state the overhead as a share of the step.
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from segmentation_factory_amd import hip  # noqa: E402
from segmentation_factory_amd.transforms import DeviceTrainTransform  # noqa: E402

S, TRIES, ITERS, ROUNDS, RATIO = 512, 10, 10, 5, 0.75
SRC_H, SRC_W = 1024, 2048
STACKS = [None, 0.5, 1.0, 2.0]                               # None: the unscaled stack
DISTINCT = 16                                                # distinct sources; a batch repeats them


def label_map(kind, seed):
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 19, (SRC_H // 64, SRC_W // 64)), np.ones((64, 64), dtype=np.int64)).astype(np.uint8)
    if kind == 'a':
        return blocks
    if kind == 'b':
        return np.full((SRC_H, SRC_W), 7, np.uint8)
    blocks[:, :SRC_W * 3 // 4] = 7
    return blocks


def windows_c(r, res_h, res_w):
    """Four windows inside the one-class part, then windows flush with the right edge (resized coordinates, no padding needed)."""
    left_max = max(res_w * 3 // 4 - S, 0)
    top = lambda: r.randint(0, max(res_h - S, 0))            # noqa: E731
    return [(top(), r.randint(0, left_max)) for _ in range(4)] + [(top(), res_w - S) for _ in range(TRIES - 3)]


def events_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step-ms', type=float, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'input_balanced_crop.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_input_balanced.py measures on the GPU'
    gen = torch.Generator(device='cuda').manual_seed(0)
    images = [torch.randint(0, 256, (SRC_H, SRC_W, 3), dtype=torch.uint8, device='cuda', generator=gen) for _ in range(DISTINCT)]
    rows = []
    for kind in 'abc':
        labels = [torch.from_numpy(label_map(kind, 10 + k)).cuda() for k in range(DISTINCT)]
        for B in (256, 4):
            imgs, lbls = [images[k % DISTINCT] for k in range(B)], [labels[k % DISTINCT] for k in range(B)]
            out = (torch.empty((B, 3, S, S), dtype=torch.float32, device='cuda'), torch.empty((B, S, S), dtype=torch.int64, device='cuda'))
            for scale in STACKS:
                kw = {} if scale is None else dict(scale_range=(scale, scale), pad_if_needed=True, label_fill=255)
                tf = DeviceTrainTransform(S, rng=random.Random(1), cat_max_ratio=RATIO, crop_tries=TRIES, **kw)
                r = random.Random(2)
                if scale is None:
                    params = [tf.draw_balanced(SRC_H, SRC_W) for _ in range(B)]
                    if kind == 'c':
                        params = [(windows_c(r, SRC_H, SRC_W), ops, flip) for _, ops, flip in params]
                    K, cand = tf._candidates([p[0] for p in params])
                    first = [(p[0][0][0], p[0][0][1], p[1], p[2]) for p in params]
                    samples, dcand = tf.pack(imgs, lbls, first, cand)
                    off_samples = tf.pack(imgs, lbls, first)
                    chosen = torch.empty(B, dtype=torch.int32, device='cuda')

                    def on():
                        hip.input_crop_select(samples, dcand, B, K, S, S, RATIO, None, 255, chosen)
                        hip.input_train(samples, B, S, S, tf.mean, tf.std, None, out[0], out[1])

                    def off():
                        hip.input_train(off_samples, B, S, S, tf.mean, tf.std, None, out[0], out[1])
                else:
                    params = [tf.draw_scaled(SRC_H, SRC_W) for _ in range(B)]
                    if kind == 'c':
                        params = [dict(p, windows=windows_c(r, p['res_h'], p['res_w'])) for p in params]
                        params = [dict(p, top=p['windows'][0][0], left=p['windows'][0][1]) for p in params]
                    K, cand = tf._candidates([p['windows'] for p in params])
                    recs, kmax = tf.pack_scaled(imgs, lbls, params)
                    hcand = (C.c_int32 * len(cand))(*cand)
                    ws = torch.empty(int(hip.lib().segf_input_train_scaled_select_ws(B, S, S, kmax, K)), dtype=torch.uint8, device='cuda')
                    chosen = torch.empty(B, dtype=torch.int32, device='cuda')

                    def on():
                        hip.input_train_scaled_select(recs, hcand, B, K, S, S, kmax, RATIO, 255, tf.mean, tf.std, None, out[0], out[1], ws, chosen)

                    def off():
                        hip.input_train_scaled(recs, B, S, S, kmax, tf.mean, tf.std, None, out[0], out[1], ws)
                assert K == TRIES + 1
                on()
                off()
                torch.cuda.synchronize()
                picks = chosen.tolist()
                t_on, t_off = [], []
                for _ in range(ROUNDS):
                    t_off.append(events_ms(off))
                    t_on.append(events_ms(on))
                m_on, m_off = statistics.median(t_on), statistics.median(t_off)
                row = dict(labels=kind, batch=B, stack='unscaled' if scale is None else f'scaled {scale}', off_ms=round(m_off, 3),
                           on_ms=round(m_on, 3), overhead_ms=round(m_on - m_off, 3), overhead_ratio=round((m_on - m_off) / m_off, 3),
                           chosen_min=min(picks), chosen_max=max(picks), chosen_mean=round(sum(picks) / B, 2),
                           max_spread=round(max((max(v) - min(v)) / statistics.median(v) for v in (t_on, t_off)), 3))
                if args.step_ms and B == 256:
                    row['share_of_step'] = round((m_on - m_off) / args.step_ms, 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
    write_profile(args, rows)


def write_profile(args, rows):
    cmd = 'python tools/bench_input_balanced.py' + (f' --step-ms {args.step_ms:g}' if args.step_ms else '')
    L = ['# Class-balanced crop choice (cat_max_ratio) in the device input pipeline', '',
         f'Measured on one MI355X by `{cmd}` (torch {torch.__version__}, {torch.cuda.get_device_name(0)}): {S} x {S} crops of '
         f'{SRC_W} x {SRC_H} sources, tries = {TRIES}, ratio {RATIO}, full jitter, median of {ROUNDS} rounds of {ITERS} calls, feature on '
         'and off alternating in one process, device events, records packed beforehand.  `off` is the plain entry point of the same '
         'build on the first window of the same draws (the parent commit\'s path, unchanged by construction).  Labels: (a) blocks, '
         'window 0 passes; (b) one class, all ten tests fail, every lane hits one counter; (c) the walk passes at the fifth window.  '
         '`overhead / off` is (on - off) / off: above 1 the choice costs more than the plain batch itself.', '',
         '| labels | batch | stack | off ms | on ms | overhead ms | overhead / off | chosen (min .. max, mean) | share of the step | max spread |',
         '|---|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        share = f"{100 * r['share_of_step']:.2f} %" if 'share_of_step' in r else '-'
        L.append(f"| ({r['labels']}) | {r['batch']} | {r['stack']} | {r['off_ms']} | {r['on_ms']} | {r['overhead_ms']} | {r['overhead_ratio']} | "
                 f"{r['chosen_min']} .. {r['chosen_max']}, {r['chosen_mean']} | {share} | {r['max_spread']} |")
    for kind in 'abc':
        sel = [r for r in rows if r['labels'] == kind]
        L += ['', f"({kind}): overhead / off {min(r['overhead_ratio'] for r in sel)} to {max(r['overhead_ratio'] for r in sel)}."]
    if args.step_ms:
        big = [r for r in rows if r['batch'] == 256]
        L += ['', f"Against the train step: `bench.py --gpus 1 --steps 20 --warmup 5` of the same session reports ms_per_step = "
                  f"{args.step_ms:g} at batch 256, 512 x 512 (the step's code is the parent commit's; the choice is no part of it).  The "
                  f"overhead of one batch-256 input call is {100 * min(r['share_of_step'] for r in big):.2f} % to "
                  f"{100 * max(r['share_of_step'] for r in big):.2f} % of that step."]
    else:
        L += ['', 'Against the train step: not measured in this run (no --step-ms given).']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(L) + '\n')


if __name__ == '__main__':
    main()
