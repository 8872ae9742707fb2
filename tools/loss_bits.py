"""Bits of the fused loss and evaluation kernels, for comparing two builds of the library.

    python tools/loss_bits.py > a.txt                                        (the in-tree build)
    SEGFAC_HIP_LIB=/path/to/other/libsegfac_hip.so python tools/loss_bits.py > b.txt
    diff a.txt b.txt

One line per case: the case id, the traced loss / evaluation kernel names (hip.trace, helpers filtered out as tests/loss_refs.py does)
and a SHA-256 over the raw bytes of every output.  These kernels are bitwise reproducible (integer atomics only), so two builds that
compute the same thing print the same file.  The cases and their inputs are those of the GPU tests, imported, not restated:
  ce_dice     every (case, dtype) of GPU_CASES of tests/loss_refs.py under its PATH_ENV switches     hash: loss, stats, lse, then dlow
  pixel_loss  SHAPES x MODES x DTYPES of tests/test_pixel_losses_gpu.py                              hash: loss, ce_map, state, then dlow
  argmax      segf_argmax_confmat with and without pred_out, (2, 19, 9, 11) at ratios 1 / 2 / 4 / 8 and (2, 150, 5, 7) -> (18, 23)
  msf, slide  the smallest shapes of tests/test_msf_eval_gpu.py / tests/test_slide_eval_gpu.py       hash: mat, hist, flag, pred, row
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import loss_refs as LR                      # noqa: E402
import msf_refs as MR                       # noqa: E402
import slide_refs as SR                     # noqa: E402
import test_loss_float64 as TL              # noqa: E402
import test_pixel_losses_gpu as TP          # noqa: E402
from test_slide_eval_gpu import GEOMS as SLIDE_GEOMS    # noqa: E402
from segmentation_factory_amd import hip    # noqa: E402

# torch.empty comes back filled (NaN / INT_MAX) rather than with whatever the allocator held: words of an output buffer that a call
# leaves unwritten (the retry flags of a path without a retry pass, say) then hash alike in every run
torch.use_deterministic_algorithms(True, warn_only=True)
torch.utils.deterministic.fill_uninitialized_memory = True


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b'none')
            continue
        torch.cuda.synchronize()
        c = t.detach().contiguous().cpu()
        h.update(f'{tuple(c.shape)}{c.dtype}'.encode())
        h.update(c.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def line(cid, kernels, sha):
    print(f'{cid} | {"; ".join(kernels)} | {sha}', flush=True)


def ce_dice():
    for c in TL.GPU_CASES:
        for k, v in c['env'].items():
            os.environ[k] = v
        hip.policy_reload()
        for dtype in LR.dtypes_of(c):
            buf, tok, tg, cw = TL._device_inputs(c, dtype, LR.inputs(c, dtype))
            geo = (c['B'], c['C'], c['h'], c['w'], c['H'], c['W'])
            go = torch.full((1,), c['go'], device='cuda')
            with hip.trace() as tf:
                loss, stats, lse = hip.ce_dice_fwd(tok, *geo, tg, LR.IGNORE, cw, c['dice'], want_lse=True)
            fwd = digest(loss, stats, lse)
            with hip.trace() as tb:
                d = hip.ce_dice_bwd(tok, *geo, tg, LR.IGNORE, cw, c['dice'], stats, go, lse=lse)
            line(f'ce_dice {c["id"]} {TL._name(dtype)}', LR.loss_kernels(tf.kernels) + LR.loss_kernels(tb.kernels), fwd + ' ' + digest(d))
        for k in c['env']:
            del os.environ[k]
        hip.policy_reload()


def pixel_loss():
    params = {'focal_025_2': (hip.PIXEL_FOCAL, 0.25, 2.0), 'focal_1_0': (hip.PIXEL_FOCAL, 1.0, 0.0)}
    go = torch.ones(1, device='cuda')
    for geom in TP.SHAPES:
        for mode in TP.MODES:
            for dtype, name in zip(TP.DTYPES, TP.IDS):
                lo, t, cw = TP._inputs(geom, mode, dtype)
                B, C, h, w, H, W = geom
                x = lo.reshape(B * h * w, C).to(dtype).cuda()
                args = (x, *geom, t.cuda(), TP.R.IGNORE, None if cw is None else cw.cuda(), *params.get(mode, (hip.PIXEL_OHEM, TP.THETA, 0.0)), 1)
                with hip.trace() as tr:
                    loss, ce_map, state = hip.pixel_loss_fwd(*args)
                    fwd = digest(loss, ce_map, state)
                    d = hip.pixel_loss_bwd(*args, ce_map, state, go)
                    bwd = digest(d)
                line(f'pixel_loss {geom} {mode} {name}', [k for k in tr.kernels if k.startswith(('pixel_loss_fwd', 'pixel_loss_bwd', 'bilinear'))],
                     fwd + ' ' + bwd)


def eval_line(cid, kernels, out):
    line(cid, kernels, digest(out['mat'], out['hist'], torch.tensor([out['flag']]), out['pred'], out.get('prob', out.get('mean'))))


def argmax():
    geoms = [(2, 19, 9, 11, 9 * r, 11 * r) for r in (1, 2, 4, 8)] + [(2, 150, 5, 7, 18, 23)]
    for B, C, h, w, H, W in geoms:
        target = MR.make_target(B, H, W, C, bad_label=200).cuda()
        for dtype, name in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
            x = MR.make_maps(B, C, [(h, w, 0)], 3.0, dtype, seed=C + H)[0].reshape(B * h * w, C).cuda()
            for want_pred in (False, True):
                mat = torch.zeros((C, C), dtype=torch.int64, device='cuda')
                hist, flag = mat.clone(), torch.zeros(1, dtype=torch.int32, device='cuda')
                pred = torch.full((B, H, W), -1, dtype=torch.int64, device='cuda') if want_pred else None
                with hip.trace() as tr:
                    hip.argmax_confmat(x, B, C, h, w, H, W, target, 255, mat, hist, flag, pred_out=pred)
                line(f'argmax {(B, C, h, w, H, W)} {name} pred_out={want_pred}', tr.kernels, digest(mat, hist, flag, pred))


def evals():
    for cid, geoms, (H, W), storage in (('1x1', [(1, 1, 0)], (1, 1), torch.float32), ('W3-w2-flip', [(2, 2, 1), (3, 2, 0)], (5, 3), torch.bfloat16)):
        B = 1 if cid == '1x1' else 2
        maps = MR.make_maps(B, 19, geoms, 3.0, storage, seed=7)
        target = torch.randint(0, 19, (B, H, W), generator=torch.Generator().manual_seed(1))
        with hip.trace() as tr:
            out = MR.run_kernel(maps, [f for _, _, f in geoms], 19, H, W, target=target)
        eval_line(f'msf {cid}', tr.kernels, out)
    for name in ('one-window', 'grid-2x3'):
        H, W, crop, stride, hw, C, pad, seed = SLIDE_GEOMS[name]
        for storage, sname in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
            ny, nx, _ = SR.windows_of(H, W, crop, stride)
            maps = SR.make_maps(2, C, ny * nx, hw[0], hw[1], storage, seed)
            with hip.trace() as tr:
                out = SR.run_kernel(maps, C, H, W, crop, stride, target=MR.make_target(2, H, W, C), ldl=C + pad)
            eval_line(f'slide {name} {sname}', tr.kernels, out)


if __name__ == '__main__':
    print(f'# {hip.LIB_PATH if os.environ.get("SEGFAC_HIP_LIB") else "in-tree build"}', file=sys.stderr)
    ce_dice()
    pixel_loss()
    argmax()
    evals()
