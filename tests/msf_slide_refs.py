"""Helpers of the multi-scale + flip sliding-window evaluation tests: the torch restatement of segf_msf_slide_argmax_confmat
(include/segfac.h), the standard case and the kernel runner.  No test lives here."""
import functools

import torch
import torch.nn.functional as F

import msf_refs
import slide_refs
from msf_refs import TIE_MARGIN, TIE_SHARE, counts, make_target, prob_atol, tie_band  # noqa: F401

STANDARD_B, STANDARD_HW = 2, (24, 40)
# ((Hs, Ws), crop, stride, (h, w), flip) of the standard case; crop / stride as asked, clamped by `clamp` as engine.slide_windows does
STANDARD_SETS = (
    ((12, 20), (16, 16), (11, 11), (3, 4), 0),       # crop clamped to a 12 x 16 window, 1 x 2 grid, outer upsampling
    ((24, 40), (16, 16), (11, 11), (4, 4), 1),       # same-size outer read, 2 x 4 grid with a moved-back last window, mirrored
    ((36, 60), (16, 16), (11, 11), (4, 4), 0),       # outer downsampling, 3 x 5 grid
    ((42, 70), (16, 16), (11, 11), (5, 5), 1),       # non-integer inner ratio, mirrored
    ((24, 40), (24, 40), (24, 40), (6, 10), 0),      # one window = the whole image (the MSF degenerate)
    ((18, 30), (16, 16), (5, 5), (16, 16), 1),       # direct inner read, 8-fold cover
)


def clamp(size, crop, stride):
    """(crop_eff, stride_eff) of engine.slide_windows, restated: the crop clamped to the image, the stride to the crop."""
    ch, cw = min(crop[0], size[0]), min(crop[1], size[1])
    return (ch, cw), (min(stride[0], ch), min(stride[1], cw))


def make_sets(B, C, geoms, storage, amp, seed0=10):
    """[dict(maps [B, nWin, h, w, C], size, crop, stride, flip)] of the geometries, set k seeded with seed0 + k."""
    sets = []
    for k, (size, crop, stride, (h, w), flip) in enumerate(geoms):
        crop, stride = clamp(size, crop, stride)
        ny, nx, _ = slide_refs.windows_of(size[0], size[1], crop, stride)
        sets.append(dict(maps=slide_refs.make_maps(B, C, ny * nx, h, w, storage, seed=seed0 + k, amp=amp), size=size, crop=crop,
                         stride=stride, flip=flip))
    return sets


def oracle(sets, H, W, dtype):
    """Per set: slide_refs.oracle at (Hs, Ws) -> .flip(3) if flagged -> F.interpolate to (H, W) unless same size -> softmax(1);
    summed in list order.  -> [B, C, H, W] `dtype`."""
    S = None
    for s in sets:
        M, _ = slide_refs.oracle(s['maps'], s['size'][0], s['size'][1], s['crop'], s['stride'], dtype)
        if s['flip']:
            M = M.flip(3)
        if tuple(s['size']) != (H, W):
            M = F.interpolate(M, size=(H, W), mode='bilinear', align_corners=False)
        p = M.softmax(1)
        S = p if S is None else S + p
    return S


def reference(sets, H, W):
    """(S64, e32): the float64 oracle and the error of the float32 restatement against it (it makes the same two resamplings and the
    same division in fp32, so it prices them)."""
    S64 = oracle(sets, H, W, torch.float64)
    e32 = (oracle(sets, H, W, torch.float32).double() - S64).abs().max().item()
    return S64, e32


@functools.lru_cache(maxsize=None)
def standard_case(C, amp, storage, seed0=10):
    """(sets, S64, e32) of the standard case.  Cached: computed once, shared, never modified."""
    H, W = STANDARD_HW
    sets = make_sets(STANDARD_B, C, STANDARD_SETS, storage, amp, seed0)
    S64, e32 = reference(sets, H, W)
    return sets, S64, e32


def device_rows(maps, C, ldl=None):
    """CPU maps [B, nWin, h, w, C] -> (device rows [B*nWin*h*w, C], h, w); ldl: row stride of the device rows (the columns beyond C
    are filled with a large value that must never be read as a class)."""
    B, nwin, h, w, _ = maps.shape
    r = maps.reshape(B * nwin * h * w, C)
    if ldl is not None and ldl != C:
        buf = torch.full((r.shape[0], ldl), 1e4, dtype=maps.dtype)
        buf[:, :C] = r
        r = buf.cuda()[:, :C]
    else:
        r = r.contiguous().cuda()
    return r, h, w


def run_kernel(sets, C, H, W, target=None, ignore_label=255, want_pred=True, want_prob=True, ldl=None, ldp=None):
    """Call hip.msf_slide_argmax_confmat on CPU sets; -> dict(prob [B, H, W, C] fp32, pred, mat, hist, flag) on the CPU."""
    from segmentation_factory_amd import hip
    B = sets[0]['maps'].shape[0]
    wsets = [(device_rows(s['maps'], C, ldl), s['size'], s['crop'], s['stride']) for s in sets]
    flips = [s['flip'] for s in sets]
    mat = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device='cuda') if want_pred else None
    prob = None
    if want_prob:
        prob = torch.full((B * H * W, ldp or C), -1.0, dtype=torch.float32, device='cuda')[:, :C]
    tg = target.cuda() if target is not None else None
    hip.msf_slide_argmax_confmat(wsets, flips, B, C, H, W, tg, ignore_label, mat, hist, flag, pred_out=pred, prob_out=prob)
    torch.cuda.synchronize()
    return dict(prob=prob.cpu().reshape(B, H, W, C) if want_prob else None, pred=pred.cpu() if want_pred else None,
                mat=mat.cpu(), hist=hist.cpu(), flag=int(flag.item()))
