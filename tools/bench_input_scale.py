"""Times the scaled training input path (segf_input_train_scaled: random scale + padded crop computed for the crop window only)
beside the unscaled one (segf_input_train) in the same process, and writes profiles/input_scale_crop.md.

    python tools/bench_input_scale.py [--step-images-per-s X] [--out profiles/input_scale_crop.md]

Batch 64, 512 x 512 crops, sources 683 x 512 and 2048 x 1024 (w x h), scales 0.5 / 1.0 / 2.0 fixed per run (scale_range = (s, s)),
full jitter.  Two timings per case, each the median of ROUNDS rounds that alternate the two paths:
  * `call`: device events around ITERS calls with the records packed beforehand (scaled: upload of the records, the table kernel,
    the crop kernel, the luma-sum and train kernels; unscaled: the luma-sum and train kernels);
  * `loader`: host clock around ITERS whole transform calls (draws, packing, upload, kernels) ending in a device synchronise.
Bytes are algorithmic, from the shapes: per crop pixel 24 (the unscaled path: 3 + 1 read, 12 + 8 written) + 8 (staged uint8 crop
written and read back: 3 + 1 each way) + the source footprint of the window (every source pixel under a tap once, 3 bytes, plus one
label byte per window pixel inside the resized image).  --step-images-per-s: the train step's images/s (the `value` of bench.py's
result line) to compare the loader against.  Needs the GPU; there is no fallback."""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from segmentation_factory_amd import hip  # noqa: E402
from segmentation_factory_amd.transforms import DeviceTrainTransform, label_table  # noqa: E402

B, S, ITERS, ROUNDS = 64, 512, 20, 5
SOURCES = [(512, 683), (1024, 2048)]                         # (h, w)
SCALES = [0.5, 1.0, 2.0]


def footprint_bytes(p, src_h, src_w):
    """Source bytes under the window of one sample (algorithmic: each touched source pixel once)."""
    rows = max(0, min(p['top'] + S, p['res_h']) - max(p['top'], 0))
    cols = max(0, min(p['left'] + S, p['res_w']) - max(p['left'], 0))
    if rows == 0 or cols == 0:
        return 0
    sr = min(src_h, math.ceil(rows * src_h / p['res_h']) + hip.resample_ksize(src_h, p['res_h']) - 1)
    sc = min(src_w, math.ceil(cols * src_w / p['res_w']) + hip.resample_ksize(src_w, p['res_w']) - 1)
    return sr * sc * 3 + rows * cols


def events_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step-images-per-s', type=float, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'input_scale_crop.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_input_scale.py measures on the GPU'
    gen = torch.Generator(device='cuda').manual_seed(0)
    lut = label_table({255: 0})
    rows = []
    for (h, w) in SOURCES:
        imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device='cuda', generator=gen) for _ in range(B)]
        lbls = [torch.randint(0, 256, (h, w), dtype=torch.uint8, device='cuda', generator=gen) for _ in range(B)]
        plain = DeviceTrainTransform(S, label_lut=lut, rng=random.Random(0))
        pparams = [plain.draw(h, w) for _ in range(B)]
        psamples = plain.pack(imgs, lbls, pparams)
        out = hip.input_train(psamples, B, S, S, plain.mean, plain.std, plain.label_lut)

        def plain_call():
            hip.input_train(psamples, B, S, S, plain.mean, plain.std, plain.label_lut, out[0], out[1])

        def plain_loader():
            plain(imgs, lbls, out=out)
        for scale in SCALES:
            tf = DeviceTrainTransform(S, label_lut=lut, rng=random.Random(1), scale_range=(scale, scale), pad_if_needed=True, label_fill=255)
            sparams = [tf.draw_scaled(h, w) for _ in range(B)]
            recs, kmax = tf.pack_scaled(imgs, lbls, sparams)
            ws = torch.empty(int(hip.lib().segf_input_train_scaled_ws(B, S, S, kmax)), dtype=torch.uint8, device='cuda')

            def scaled_call():
                hip.input_train_scaled(recs, B, S, S, kmax, tf.mean, tf.std, tf.label_lut, out[0], out[1], ws)

            def scaled_loader():
                tf(imgs, lbls, out=out)
            for fn in (plain_call, scaled_call, plain_loader, scaled_loader):            # warm-up of every timed shape
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ('pc', 'sc', 'pl', 'sl')}
            for _ in range(ROUNDS):                                                      # alternate the two paths
                t['pc'].append(events_ms(plain_call))
                t['sc'].append(events_ms(scaled_call))
                t['pl'].append(host_ms(plain_loader))
                t['sl'].append(host_ms(scaled_loader))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in t.items()}
            gb_plain = B * S * S * 24 / 1e9
            gb_scaled = (B * S * S * 32 + sum(footprint_bytes(p, h, w) for p in sparams)) / 1e9
            row = dict(source=f'{w} x {h}', scale=scale, kmax=kmax, workspace_MB=round(ws.numel() / 2 ** 20, 1),
                       unscaled_call_ms=round(med['pc'], 3), scaled_call_ms=round(med['sc'], 3),
                       unscaled_call_img_s=round(B / med['pc'] * 1e3), scaled_call_img_s=round(B / med['sc'] * 1e3),
                       call_ratio=round(med['pc'] / med['sc'], 3),
                       unscaled_loader_img_s=round(B / med['pl'] * 1e3), scaled_loader_img_s=round(B / med['sl'] * 1e3),
                       loader_ratio=round(med['pl'] / med['sl'], 3),
                       unscaled_GB=round(gb_plain, 3), scaled_GB=round(gb_scaled, 3), scaled_GB_per_s=round(gb_scaled / med['sc'] * 1e3, 1),
                       max_spread=round(max(spread.values()), 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    write_profile(args, rows)


def write_profile(args, rows):
    cmd = 'python tools/bench_input_scale.py' + (f' --step-images-per-s {args.step_images_per_s:g}' if args.step_images_per_s else '')
    L = ['# Scaled training input path: random scale + padded crop for the crop window only', '',
         f'Measured on one MI355X by `{cmd}` (torch {torch.__version__}, {torch.cuda.get_device_name(0)}): batch {B}, {S} x {S} crops, '
         f'full jitter, median of {ROUNDS} rounds of {ITERS} calls, the two paths alternating in one process.  `call`: device events, '
         'records packed beforehand; `loader`: host clock around the whole transform call (draws, packing, upload, kernels) ending in a '
         'synchronise.  Ratios are unscaled time / scaled time of the same build: below 1 the scaled path is slower.  Bytes are '
         'algorithmic (24 per crop pixel for the unscaled path; 32 per crop pixel plus the source footprint of the window for the '
         'scaled one).', '',
         '| source (w x h) | scale | taps | workspace MB | unscaled call ms | scaled call ms | scaled call images/s | call ratio | '
         'unscaled loader images/s | scaled loader images/s | loader ratio | scaled GB | scaled GB/s | max spread |',
         '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        L.append(f"| {r['source']} | {r['scale']} | {r['kmax']} | {r['workspace_MB']} | {r['unscaled_call_ms']} | {r['scaled_call_ms']} | "
                 f"{r['scaled_call_img_s']} | {r['call_ratio']} | {r['unscaled_loader_img_s']} | {r['scaled_loader_img_s']} | "
                 f"{r['loader_ratio']} | {r['scaled_GB']} | {r['scaled_GB_per_s']} | {r['max_spread']} |")
    slow = min(rows, key=lambda r: r['scaled_loader_img_s'])
    L += ['', f"Against the unscaled path of the same build: call ratio {min(r['call_ratio'] for r in rows)} to "
              f"{max(r['call_ratio'] for r in rows)}, loader ratio {min(r['loader_ratio'] for r in rows)} to "
              f"{max(r['loader_ratio'] for r in rows)}.  The workspace is the same for every scale of a crop size with the same tap "
              f"count bound: it holds tables and two staged uint8 planes, never a resized image."]
    if args.step_images_per_s:
        x = args.step_images_per_s
        verdict = ('The scaled loader is FASTER than the train step in every case: it does not bound training.'
                   if slow['scaled_loader_img_s'] > x else
                   f"The scaled loader is SLOWER than the train step in its slowest case ({slow['source']}, scale {slow['scale']}): there the "
                   f"loader, not the step, bounds training.")
        L += ['', f"Against the train step: `bench.py --gpus 1 --steps 20 --warmup 5` reports {x:g} images/s for the step (run on the same "
                  f"machine right before this tool; the step's code is the parent commit's, the scaled path is no part of it); the slowest scaled "
                  f"loader case ({slow['source']}, scale {slow['scale']}) delivers {slow['scaled_loader_img_s']} images/s.  {verdict}"]
    else:
        L += ['', 'Against the train step: not measured in this run (no --step-images-per-s given).']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(L) + '\n')


if __name__ == '__main__':
    main()
