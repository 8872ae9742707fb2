#!/usr/bin/env python3
"""Headline benchmark: images/sec/GPU for one full training step (zero_grad + forward + fused upsample/CE/Dice
loss + backward + AGC/AdamW step) of SegFormer-B0 *as the reference builds it* (MiT-B0 + 768-wide SegFormerHead,
150 classes) at 512x512, bf16 storage / fp32 accumulate, synthetic data resident in HBM.

  python bench.py --gpus 1 --steps 20 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      bench.py --gpus N --steps K --warmup W          (one rank per GPU; each rank replays its hipGraph, whose in-graph event
                                                       nodes release the bucketed RCCL gradient exchange on a communication
                                                       stream while the backward is still running; then the fused optimizer)

Prints ONE JSON line on rank 0: the headline figure of the timed steps (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`) and the run's configuration.  A plain run does nothing else: set-up, warm-up, the timed steps, the optional
--dump-outputs files, the line.

  --dump-outputs DIR   after the timed steps, what the last one handed its caller as DIR/<name>.npy (float32; see dump_outputs)
  --full               also the secondary figures, each measured by runs of its own after the timed steps: forward + loss + backward
                       only, a `roofline` object for the dominant kernel (ce_dice_bwd_band_kernel; HIP-event timed on its launch
                       stream; `roofline_gemm` = the heaviest HBM-bound GEMM launch), the input pipeline, the other BASELINE
                       configurations / train loop / evaluate legs (tools/bench_legs.py; --no-extra-legs drops them) and a
                       `cpu_baseline` object (the CPU oracle port of the reference path timed on this host's cores, bounded sample;
                       --no-cpu-baseline drops it)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK = 2.5e15       # dense bf16 MFMA peak, FLOP/s (MI355X_MICROARCH.md)
HBM_PEAK = 8.0e12             # HBM3E peak, B/s (MI355X_MICROARCH.md; ~6.3e12 achievable)
FWD_GFLOP_PER_IMG = 89.05     # reference graph as written, forward
NC, H, W = 150, 512, 512
# BASELINE.json configs: backbone, head, classes, height, width
CONFIGS = {'cfg2': ('MiT-B0', 'SegFormerHead', 150, 512, 512), 'cfg3': ('ConvNeXt', 'UPerHead', 150, 512, 512),
           'cfg4': ('MiT-B2', 'SegFormerHead', 19, 1024, 2048), 'cfg5': ('convnextv2_large', 'UPerHead', 171, 640, 640)}


def synthetic_batch(batch, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((batch, 3, H, W), dtype=np.float32)
    lbl = rng.integers(0, NC, (batch, H, W), dtype=np.int64)
    lbl[:, :8] = 255
    lbl[rng.random((batch, H, W)) < 0.02] = 255
    return torch.from_numpy(img), torch.from_numpy(lbl)


def numpy_seed_weights(model, seed):
    """std 0.02 for the linear (2-D) weights, fan-out normal for the convolutions (mit.py:27-40), vectors (norm scales,
    biases, layer scales) as the modules' own initialisers left them -- all from numpy.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.ndim == 2:
                p.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape), dtype=np.float32) * 0.02)))
            elif p.ndim == 4:
                groups = p.shape[0] if p.shape[1] == 1 else 1                  # [O, 1, k, k] = depthwise
                fan_out = p.shape[2] * p.shape[3] * p.shape[0] // groups
                std = float(np.sqrt(2.0 / max(fan_out, 1)))
                p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape), dtype=np.float32) * std))


# sources a kernel's counter traffic depends on (its own files + the shared headers + the build flags): a gemm.hip edit must not
# void the loss kernel's figure and vice versa
# per-GPU batch of each BASELINE configuration, sized for 288 GB of HBM by a same-box sweep (profiles/r05_batch_sweep.txt): 38 / 41 / 84 /
# 65 GB peak; powers of two fill the tile grids (cfg2: 192 and 320 are slower than 128 and 256)
DEFAULT_BATCH = {'cfg2': 256, 'cfg3': 64, 'cfg4': 32, 'cfg5': 32}
KERNEL_SOURCES = {'loss_bwd': ('loss.hip', 'loss_band.hip', 'loss_geom.h', 'common.h', 'Makefile'),
                  'gemm_pro': ('gemm.hip', 'common.h', 'colreduce.h', 'Makefile')}


def kernel_source_hash(which=None):
    """Hash of the HIP sources behind one roofline object ('loss_bwd' / 'gemm_pro'; None -> {name: hash}): stamps
    profiles/pmc_traffic_*.json so that a counter file measured on other kernel code is never reported as this run's traffic."""
    import hashlib
    csrc = os.path.join(ROOT, 'segmentation_factory_amd', 'csrc')
    out = {}
    for key, names in KERNEL_SOURCES.items():
        h = hashlib.sha256()
        for n in sorted(names):
            h.update(n.encode())
            with open(os.path.join(csrc, n), 'rb') as fh:
                h.update(fh.read())
        out[key] = h.hexdigest()[:16]
    return out if which is None else out[which]


DUMP_MAX_ELEMS = 7 << 20      # per dumped array (float32: 28 MiB; params + grads + loss stay under 64 MB)


def dump_outputs(dirname, loss, params, grads):
    """--dump-outputs: what the timed step hands its caller after the last timed step, as float32 DIR/<name>.npy -- loss.npy (the step's
    loss), params.npy (the updated parameters) and grads.npy (the gradients the optimizer consumed), parameters concatenated in the
    optimizer's order.  An array longer than DUMP_MAX_ELEMS is written as a fixed sample: the sorted distinct indices of
    DUMP_MAX_ELEMS draws from numpy default_rng(0), which depend on the array's length only."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {'loss': loss.detach().float().reshape(1),
              'params': torch.cat([t.detach().reshape(-1).float() for t in params]),
              'grads': torch.cat([t.detach().reshape(-1).float() for t in grads])}
    for name, t in arrays.items():
        if t.numel() > DUMP_MAX_ELEMS:
            idx = np.unique(np.random.default_rng(0).integers(0, t.numel(), DUMP_MAX_ELEMS))
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(dirname, name + '.npy'), t.cpu().numpy())


def cpu_baseline(sample_batch=2, timed_steps=3, loop_timed_steps=2):
    """The oracle (CPU restatement of the reference path, validated bit-exact against the imported reference in the build
    container) timed on this host, SURVEY section 8(d): same synthetic batch, 1 warm-up + 3 timed steps of forward + CE/Dice +
    backward with the reference's B x C Python Dice loop (util/losses.py:141-170: its cost structure), and next to it the
    same with the vectorised closed-form Dice."""
    from oracle import loss as OL, nets as ON, weights as OW
    # the GPU box exposes 256 logical CPUs but a 1-GPU job owns a 16-core share.  Measured on the box (tools/probe/cpu_threads_probe.py,
    # profiles/r05_cpu_threads.txt; the same step with the vectorised Dice): 16 threads 1.05 images/s, 32 threads 0.93, 64 threads 0.81 --
    # more threads than the share are SLOWER, so the cap is the fastest setting, not a handicap
    ncores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(ncores)
    sd = OW.make_state_dict('MiT-B0', 'SegFormerHead', 150, 0, lively=False)
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and not k.endswith(('running_mean', 'running_var')))
          for k, v in sd.items()}
    x, y = OW.synthetic_batch(sample_batch, 512, 512, 150, 0)

    def step(crit):
        for v in sd.values():
            v.grad = None
        o, _ = ON.model_forward(sd, x, 'MiT-B0', 'SegFormerHead', training=True)
        crit(o, y, None, num_classes=150, dice=True, ignore_index=255).backward()

    def timed(crit, n):
        step(crit)                                   # warm-up (allocator, thread pool, first-touch)
        t0 = time.time()
        for _ in range(n):
            step(crit)
        return (time.time() - t0) / n
    t_loop = timed(OL.criterion_loops, loop_timed_steps)     # ~28 s per step on the GPU box's 16-thread share: two timed steps
    t_vec = timed(OL.criterion_closed_form, timed_steps)
    cpu_model = ''
    try:
        with open('/proc/cpuinfo') as fh:
            cpu_model = next((l.split(':', 1)[1].strip() for l in fh if l.startswith('model name')), '')
    except OSError:
        pass
    return {"value": round(sample_batch / t_loop, 4), "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 warm-up + {loop_timed_steps} timed steps of fwd + CE/Dice (reference's B x C Python loop) + bwd, batch {sample_batch}, "
                      f"512x512, 150 classes, fp32: {t_loop:.2f} s/step",
            "vectorised_dice_value": round(sample_batch / t_vec, 4),
            "vectorised_dice_sample": f"1 warm-up + {timed_steps} timed steps with the closed-form (vectorised) Dice: {t_vec:.2f} s/step",
            "os_cpu_count": os.cpu_count(), "torch_threads": torch.get_num_threads(), "cpu_model": cpu_model}


def extra_legs(budget_s):
    """What the headline line does not show, measured by THIS command so that the driver observes it: the other BASELINE.json configs
    (cfg3 / cfg4 / cfg5, cfg5 with fp8, cfg2 at the reference's default batch 4 and at 16), the loop a user runs
    (engine.train_one_epoch with --hip-graph over the device-side loader) against the replay-only rate, and engine.evaluate at the
    reference's default --val_batch_size 1 and at 32 (/root/reference/train_gpu.py:71-72, engine.py:36-56,74-104).  One child process
    per leg (tools/bench_legs.py), each under a timeout; a leg that fails is reported as such and never costs the headline line."""
    import subprocess
    legs = [('other_configs', ['config', 'cfg3']), ('other_configs', ['config', 'cfg3', '--fp8']), ('other_configs', ['config', 'cfg4']),
            ('other_configs', ['config', 'cfg5']), ('other_configs', ['config', 'cfg5', '--fp8']),
            ('other_configs', ['config', 'cfg2', '--batch', '4', '--steps', '40', '--warmup', '10']),
            ('other_configs', ['config', 'cfg2', '--batch', '16', '--steps', '20', '--warmup', '5']),
            ('other_configs', ['config', 'cfg2', '--batch', '128', '--steps', '20', '--warmup', '5']),
            ('train_loop', ['train_loop', '--batch', '256', '--steps', '10', '--epochs', '2']),
            ('train_loop', ['train_loop', '--batch', '4', '--steps', '100', '--epochs', '2']),
            ('train_loop', ['default_cli', '--batch', '4', '--steps', '50', '--epochs', '2']),
            ('eval', ['eval', '--batch', '1', '--steps', '100']), ('eval', ['eval', '--batch', '32', '--steps', '10'])]
    res = {'other_configs': [], 'train_loop': [], 'eval': []}
    t0 = time.time()
    for key, argv in legs:
        left = budget_s - (time.time() - t0)
        tag = ' '.join(argv)
        if left < 8:
            res[key].append({'leg': tag, 'skipped': f'legs budget of {budget_s:.0f} s used up'})
            continue
        t1 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'bench_legs.py')] + argv, capture_output=True, text=True,
                               timeout=min(left, 90.0))
            line = next((l for l in r.stdout.splitlines() if l.startswith('LEG_JSON ')), None)
            if r.returncode == 0 and line:
                d = json.loads(line[len('LEG_JSON '):])
                d['leg_wall_s'] = round(time.time() - t1, 1)
                res[key].append(d)
            else:
                res[key].append({'leg': tag, 'error': (r.stderr or r.stdout)[-400:]})
        except subprocess.TimeoutExpired:
            res[key].append({'leg': tag, 'error': 'timeout'})
    res['extra_legs_wall_s'] = round(time.time() - t0, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None, help='per-GPU batch, default 256 / 64 / 32 / 32 for cfg2 / cfg3 / cfg4 / cfg5 (BASELINE.json does not fix it; 256 x 512^2 peaks at ~44 of 288 GB; same box: 128: -2.6 %%, 192: -3 %%, 320: -1.8 %% -- '
                    'powers of two fill the tile grids; profiles/r05_batch_sweep.txt)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--full', action='store_true', help='also the secondary figures (fwd+loss+bwd only, rooflines, input pipeline, extra legs, '
                                                        'CPU baseline), each measured after the timed steps')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write the last timed step\'s loss / updated parameters / gradients '
                                                                         'as DIR/<name>.npy (float32)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-optimizer', action='store_true', help='time forward+loss+backward only')
    ap.add_argument('--config', default='cfg2', choices=sorted(CONFIGS),
                    help='BASELINE.json configs as the reference builds them; cfg2 = SegFormer-B0 (headline)')
    ap.add_argument('--eager', action='store_true', help='per-kernel launches + torch DDP instead of the hipGraph step')
    ap.add_argument('--copy-inputs', action='store_true', help='copy the batch into the captured step\'s input buffers every step '
                                                                 '(default: it already sits there, as the device input pipeline delivers it)')
    ap.add_argument('--fp8', action='store_true', help='cfg3 / cfg5: the UPerHead 3x3 convolutions and the ConvNeXt block MLPs on fp8 operands in all three '
                                                      'products (forward e4m3 x e4m3, gradients e5m2; set_fp8)')
    ap.add_argument('--no-extra-legs', action='store_true', help='with --full: skip the secondary legs (other BASELINE configs, train loop, evaluate)')
    ap.add_argument('--legs-budget-s', type=float, default=210.0, help='wall-clock budget for the secondary legs; legs that do not fit are listed as skipped')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    if args.batch is None:
        args.batch = DEFAULT_BATCH[args.config]

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    assert torch.cuda.is_available(), 'bench.py needs MI355X GPUs (there is no CPU fallback)'
    # SEGFAC_DIST_BACKEND=gloo lets several ranks share one GPU (RCCL refuses duplicate devices): used to exercise the N>1 code
    # path on a 1-GPU box; the driver's multi-GPU runs use the default 'nccl' (= RCCL on ROCm), one rank per GPU
    backend = os.environ.get('SEGFAC_DIST_BACKEND', 'nccl')
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group(backend, init_method='env://')
    dev = torch.device('cuda', local)

    from segmentation_factory_amd import SegmentationModel, criterion_lowres, hip
    from segmentation_factory_amd.backbones import TokenMap
    from segmentation_factory_amd.optim import FusedAGCAdamW, NativeScaler, param_groups_weight_decay

    from segmentation_factory_amd.graph import GraphedTrainStep
    torch.manual_seed(1234)          # identical initial weights on every rank (rank 0's are broadcast anyway)
    dtype = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    global NC, H, W
    bb_name, head_name, NC, H, W = CONFIGS[args.config]
    core = SegmentationModel(bb_name, num_classes=NC, seg_head=head_name, compute_dtype=dtype).to(dev).train()
    if args.fp8:
        core.set_fp8(True)
    numpy_seed_weights(core, 0)      # weights from numpy's generator (the same on every box and rank), not from torch's RNG order
    opt = FusedAGCAdamW(param_groups_weight_decay(core, 0.025), lr=2e-4)
    x, y = synthetic_batch(args.batch, seed=rank)
    x, y = x.to(dev), y.to(dev)

    def loss_fn(model, img, lbl):
        lo = model.forward_lowres(img)
        return criterion_lowres(lo, lbl, (H, W), None, num_classes=NC, dice=True, ignore_index=255)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # Dominant kernel of the step by GPU time (profiles/r02*_kernel_stats.csv): ce_dice_bwd_band_kernel (loss_band.hip), the fused
    # transposed-upsample + softmax + CE/Dice backward (one launch per step).  Its algorithmic HBM traffic is tiny -- it is
    # bound by the exponentials per (full-resolution pixel, class) on the VALU (the interpolation and the tap scatter run on
    # the matrix pipe), not by HBM or MFMA; the roofline leg prices it in bytes against HBM as the contract asks and states the
    # transcendental rate next to it.  The heaviest GEMM launch (the HBM-bound
    # classifier GEMM) is reported next to it.
    hq, wq = H // 4, W // 4
    M, N, K = args.batch * hq * wq, NC, 768
    loss_key = ('ce_dice_bwd', args.batch, NC, hq, wq, H, W)
    ld = (NC + 31) // 32 * 32 if head_name == 'SegFormerHead' else (NC + 7) // 8 * 8      # class rows as the head pads them
    gemm_key = ('gemm', 0, M, ld, K)
    if args.eager:
        scaler = NativeScaler()
        model = core
        if world > 1:
            model = torch.nn.parallel.DistributedDataParallel(core, device_ids=[local], gradient_as_bucket_view=True)

        def step(with_opt=True):
            opt.zero_grad(set_to_none=True)
            if world > 1:
                data, (b_, h_, w_) = model(x, lowres=True)
                loss = criterion_lowres(TokenMap(data, b_, h_, w_), y, (H, W), None, num_classes=NC, dice=True, ignore_index=255)
            else:
                loss = loss_fn(core, x, y)
            if with_opt:
                scaler(loss, opt, clip_grad=0.02, clip_mode='agc', parameters=core.parameters())   # engine.py:52-53
            else:
                loss.backward()
            return loss
    else:
        # zero_grad + forward + CE/Dice + backward + gradient gather replayed as ONE hipGraph; the RCCL all-reduce of
        # the flat gradient buffer and the fused AGC/AdamW kernel follow it (segmentation_factory_amd/graph.py)
        gs = GraphedTrainStep(core, opt, loss_fn, (x, y), clip_grad=0.02, clip_mode='agc')
        # the synthetic batch sits in the captured step's input buffers (zero-copy feed, the way the device input pipeline delivers
        # batches: transforms.DeviceBatchLoader.bind_output); --copy-inputs re-copies it from a second tensor every step
        feed = (x, y) if args.copy_inputs else tuple(gs.static_inputs)

        def step(with_opt=True):
            return gs.step(*feed) if with_opt else gs.forward_backward(*feed)

    with_opt = not args.no_optimizer
    for _ in range(args.warmup):
        step(with_opt)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step(with_opt)
    sync()
    elapsed = time.perf_counter() - t0
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = tmax.item()
    final_loss = loss.item()
    if args.dump_outputs and rank == 0:
        # the optimizer's per-parameter views of its flat parameter / gradient buffers (graphed and eager path alike)
        dump_outputs(args.dump_outputs, loss, opt._params, opt._grad_views)
    if args.full:
        # secondary figure: forward + loss + backward only (the metric's literal wording), same session
        for _ in range(2):
            step(False)
        sync()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step(False)
        sync()
        fb = time.perf_counter() - t1
        # roofline leg: the same C-ABI calls on the same shapes, HIP-event timed on the launch stream right after the timed
        # region (launches inside a graph replay cannot be bracketed by events; the rocprofv3 summary of this command under
        # profiles/ gives the in-graph durations of the same launches)
        lo_ = torch.randn(M, ld, device=dev).to(dtype)[:, :NC]
        loss_, stats_, lse_ = hip.ce_dice_fwd(lo_, args.batch, NC, hq, wq, H, W, y, 255, None, True, want_lse=True)   # as the step runs it
        go_ = torch.ones(1, device=dev)
        A_ = torch.randn(M, K, device=dev).to(dtype)
        W_ = torch.zeros(ld, K, device=dev, dtype=dtype)
        b_ = torch.zeros(ld, device=dev)
        # the classifier product as it runs INSIDE the step: segf_gemm_pro, BatchNorm + ReLU + Dropout2d applied to the operand on
        # its way into LDS (gemm_bf16_big_kernel<0, bf16, false, PRO=true>), not the plain segf_gemm of the same shape
        rps_ = hq * wq
        use_pro = dtype == torch.bfloat16 and hip.gemm_pro_supported(dtype, 0, M, ld, K, rps_)
        sc_ = torch.ones(args.batch, K, device=dev)
        sh_ = torch.zeros(args.batch, K, device=dev)
        with hip.KernelTimer(lambda k: k in (loss_key, gemm_key)) as kt:
            for _ in range(max(args.steps, 5)):
                hip.ce_dice_bwd(lo_, args.batch, NC, hq, wq, H, W, y, 255, None, True, stats_, go_, lse=lse_)
                if use_pro:
                    hip.gemm_pro(0, A_, W_, M, ld, K, sc_, sh_, rps_, 1, bias=b_)
                else:
                    hip.gemm(0, A_, W_, M, ld, K, bias=b_)
        esz = A_.element_size()
        # SURVEY 8(d), loss kernel: low-res logits read + their gradient written (NC classes, not the padded row) + int64 labels read
        loss_bytes = args.batch * (2 * hq * wq * NC * esz + H * W * 8)
        loss_bytes_padded = args.batch * (2 * hq * wq * ld * esz + H * W * 8)      # what the rows occupy in memory (class pad columns)
        loss_exps = float(args.batch) * H * W * (16 * ((NC + 15) // 16)) * (8.0 / 7.0) * (17.0 / 16.0)   # per pixel and padded class; band sweep: 8 cells per 7 tap columns, one lead-in row per 16-row segment
        gemm_bytes = esz * (M * K + ld * K + M * ld)
        del A_, W_, lo_

        # input-pipeline leg: one batch of the reference's train transform stack (crop, Pillow colour jitter, flip,
        # ToTensor, Normalize, label table) from decoded uint8 images resident in HBM -- reported beside the step, not part of `value`
        inp = None
        if rank == 0 and H % 4 == 0:
            import random as _random
            from segmentation_factory_amd.transforms import DeviceTrainTransform, label_table
            gen_ = torch.Generator(device=dev).manual_seed(0)
            srcs_ = [(H + 40 + (k % 7) * 13, W + 60 + (k % 5) * 29) for k in range(args.batch)]
            imgs_ = [torch.randint(0, 256, (h_, w_, 3), dtype=torch.uint8, device=dev, generator=gen_) for h_, w_ in srcs_]
            lbls_ = [torch.randint(0, 256, (h_, w_), dtype=torch.uint8, device=dev, generator=gen_) for h_, w_ in srcs_]
            tr_ = DeviceTrainTransform((H, W), label_lut=label_table({255: 0}, dev), device=dev, rng=_random.Random(0))
            smp_ = tr_.pack(imgs_, lbls_, [tr_.draw(h_, w_) for h_, w_ in srcs_])
            oi_, ol_ = hip.input_train(smp_, args.batch, H, W, tr_.mean, tr_.std, tr_.label_lut)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(10):
                hip.input_train(smp_, args.batch, H, W, tr_.mean, tr_.std, tr_.label_lut, oi_, ol_)
            ev1.record()
            torch.cuda.synchronize()
            inp_ms = ev0.elapsed_time(ev1) / 10
            inp_bytes = args.batch * H * W * 24                      # 3 + 1 bytes read, 12 + 8 written per output pixel
            inp = {"kernels": "input_lsum_kernel + input_train_kernel (segf_input_train)", "ms_per_batch": round(inp_ms, 4),
                   "images_per_sec": round(args.batch / inp_ms * 1e3), "algorithmic_bytes_per_batch": inp_bytes,
                   "achieved_GBps": round(inp_bytes / inp_ms / 1e6, 1), "frac_of_hbm_peak": round(inp_bytes / (inp_ms * 1e-3) / HBM_PEAK, 4),
                   "note": "bit-exact against Pillow + torch CPU (tests/test_input_pipeline.py); sources ~(H+80) x (W+120) uint8"}
            del imgs_, lbls_, oi_, ol_

        # HBM traffic per launch from the PMC counters (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of THIS command,
        # FETCH_SIZE doubled: gfx950 counts a 128-B request as 64 B; committed under profiles/): reported only for the batch it was measured at
        traffic, traffic_note = {}, {}
        try:
            with open(os.path.join(ROOT, 'profiles', f'pmc_traffic_b{args.batch}.json')) as fh:
                pmc = json.load(fh)
            have = pmc.get('source_hashes') or {}
            now = kernel_source_hash()
            usable = pmc.get('batch') == args.batch and args.config == 'cfg2' and args.dtype == 'bf16'
            for key in KERNEL_SOURCES:
                if not usable:
                    traffic_note[key] = 'no counter file for this batch / configuration'
                elif have.get(key) != now[key]:
                    traffic_note[key] = (f"profiles/pmc_traffic_b{args.batch}.json was measured on other sources of this kernel "
                                         f"(hash {have.get(key)}, now {now[key]}): not reported")
                else:
                    traffic_note[key] = f"rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes, kernel sources {now[key]}"
            for kname, v in pmc['kernels'].items():
                if kname.startswith('ce_dice_bwd') and traffic_note.get('loss_bwd', '').startswith('rocprofv3'):
                    traffic['loss_bwd'] = max(traffic.get('loss_bwd', 0), v['total_bytes'])      # (the retry kernel shares the prefix and moves no data)
                if kname.startswith('gemm_bf16_big_kernel<0') and traffic_note.get('gemm_pro', '').startswith('rocprofv3'):
                    targs = [t.strip() for t in kname[kname.index('<') + 1:kname.rindex('>')].split(',')]    # layout, out type, CONV, PRO, SHAPE, DEEP
                    if len(targs) > 3 and targs[3] == 'true':
                        traffic['gemm_pro'] = max(traffic.get('gemm_pro', 0), v['total_bytes'])
        except (OSError, ValueError, KeyError):
            pass
        for key in KERNEL_SOURCES:
            traffic_note.setdefault(key, 'no counter file for this batch / configuration')
    if rank == 0:
        ips = world * args.batch * args.steps / elapsed
        out = {
            "metric": "images/sec/GPU fwd+bwd SegFormer-B0 512x512 bf16; mIoU parity vs CPU ref" if args.config == 'cfg2'
                      else f"images/sec fwd+bwd {bb_name}+{head_name} {H}x{W} bf16",
            "value": round(ips, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("SegFormer-B0 (MiT-B0 + 768-wide SegFormerHead as the reference builds it)" if args.config == 'cfg2'
                                    else f"{bb_name} + 768-wide {head_name} (BASELINE {args.config} model)") +
                                   f", {NC} classes, {H}x{W}, " +
                                   ("full train step (zero_grad+fwd+CE/Dice+bwd+AGC/AdamW)" if with_opt else "forward+loss+backward only"),
                       "per_gpu_batch": args.batch, "global_batch": args.batch * world, "parallelism": f"dp{world}",
                       "init": "random, numpy default_rng(0): std 0.02 normal for linears, fan-out normal for convolutions (SURVEY 8d)", "loss_after": round(final_loss, 4),
                       "fp8": bool(args.fp8),
                       "inputs": "resident in HBM" + ("; copied into the captured step's input buffers every step" if (args.copy_inputs or args.eager)
                                                       else " in the captured step's input buffers (zero-copy feed)"),
                       "launch": "eager" if args.eager else "hipGraph(zero_grad+fwd+loss+bwd+grad gather) + RCCL all-reduce + fused AGC/AdamW"},
            "images_per_sec_per_gpu": round(ips / world, 2),
            "peak_hbm_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 1),
            "reference_graph_tflops_equivalent": round(3 * FWD_GFLOP_PER_IMG * 1e9 * ips / 1e12, 1) if args.config == 'cfg2' else None,
            # whole-step view with SURVEY section 8(d)'s algorithmic bytes (580 MB per image fwd+bwd at cfg2: every GEMM-class
            # output written once / read once per pass, bf16) -- the per-kernel rooflines below are the graded ones
            "step_algorithmic_hbm": ({"bytes_per_image": 580e6, "achieved_GBps": round(580e6 * ips / world / 1e9, 1),
                                      "frac_of_peak": round(580e6 * ips / world / HBM_PEAK, 4)} if args.config == 'cfg2' else None),
        }
        if args.full:
            summ = kt.summary()
            nl, avg_ms = summ.get(loss_key, (0, float('nan')))
            ng, gemm_ms = summ.get(gemm_key, (0, float('nan')))
            out["fwd_loss_bwd_only_images_per_sec"] = round(world * args.batch * args.steps / fb, 2)
            out.update({
                "roofline": {"kernel": "ce_dice_bwd_band_kernel (dominant kernel by GPU time): fused transposed upsample + softmax + CE/Dice "
                                       f"backward, low-res logits [B,{hq},{wq},{ld}] -> d logits, labels int64 [B,{H},{W}]",
                             "bound": "hbm", "achieved": round(loss_bytes / (avg_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                             "frac": round(loss_bytes / (avg_ms * 1e-3) / HBM_PEAK, 4), "traffic": traffic.get('loss_bwd'), "traffic_source": traffic_note['loss_bwd'],
                             "traffic_over_algorithmic": round(traffic['loss_bwd'] / loss_bytes, 3) if traffic.get('loss_bwd') else None,
                             "launches_timed": nl, "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": loss_bytes,
                             "padded_row_bytes_per_launch": loss_bytes_padded,
                             "note": "VALU-issue-bound, not HBM-bound: one v_exp_f32 per (full-resolution pixel, class) plus ~3.6 other VALU "
                                     "instructions (ISA count: 149 VALU + 41 transcendental + 20 MFMA per 16-pixel cell; the softmax normalisation arrives as the "
                                     "forward's per-pixel log-sum, +64 B per cell, not counted in the algorithmic bytes); interpolation / tap scatter on MFMA.  exp_per_second = %.3e (v_exp_f32 issue peak ~2.0e13/s)"
                                     % (loss_exps / (avg_ms * 1e-3))},
                "roofline_gemm": {"kernel": "gemm_bf16_big_kernel<0, bf16, false, PRO=true, SHAPE=1, DEEP=true> (segf_gemm_pro, the in-graph variant; narrow 64x80 wave tiles, three K steps of the streamed operand in flight, packed operand prologue): classifier 1x1 conv "
                                            f"[B*{hq}*{wq},768]x[768,{ld}] with BatchNorm + ReLU + Dropout2d applied on the operand load" if use_pro else
                                            f"gemm_bf16_big_kernel<0>: classifier 1x1 conv [B*{hq}*{wq},768]x[768,{ld}]",
                                  "bound": "hbm", "achieved": round(gemm_bytes / (gemm_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK / 1e9,
                                  "unit": "GB/s", "frac": round(gemm_bytes / (gemm_ms * 1e-3) / HBM_PEAK, 4),
                                  "traffic": traffic.get('gemm_pro'), "traffic_source": traffic_note['gemm_pro'],
                                  "traffic_over_algorithmic": round(traffic['gemm_pro'] / gemm_bytes, 3) if traffic.get('gemm_pro') else None,
                                  "launches_timed": ng,
                                  "avg_launch_ms": round(gemm_ms, 4), "algorithmic_bytes_per_launch": gemm_bytes,
                                  "flops_per_launch": 2.0 * M * ld * K},
            })
            if args.config != 'cfg2':
                # the loss kernel is NOT what carries these steps (cfg3 / cfg5: the UPerHead 3x3 implicit GEMMs, 68 % / 37 % of the GPU time;
                # cfg4: head-dim-64 attention, 36 %): `roofline` prices that config's own dominant kernel, the loss kernel moves aside
                sys.path.insert(0, os.path.join(ROOT, 'tools'))
                from bench_legs import dominant_kernel
                out["roofline_loss"] = out["roofline"]
                gs = step = None
                torch.cuda.empty_cache()
                out["roofline"] = dominant_kernel(args.config, args.batch, NC, H, W, args.fp8)
            if inp is not None:
                out["input_pipeline"] = inp
            # (never under a profiler: its preloaded library has initialised the GPU in this process, and the legs' child processes are
            # not started from a profiled process)
            profiled = 'rocprofiler' in os.environ.get('LD_PRELOAD', '') or any(k.startswith(('ROCPROF', 'ROCP_')) for k in os.environ)
            if world == 1 and not args.no_extra_legs and not profiled and args.config == 'cfg2' and not args.eager:
                # free this process's share of the HBM first: the children build their own models and graphs
                gs = None
                torch.cuda.empty_cache()
                out.update(extra_legs(args.legs_budget_s))
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
