"""Helpers of the sliding-window evaluation tests: the torch restatement of segf_slide_argmax_confmat (include/segfac.h), the
derived tolerance and the kernel runner.  No test lives here."""
import functools

import torch
import torch.nn.functional as F

from msf_refs import counts, make_target  # noqa: F401   (the counting restatement and the label maker are the MSF tests')

AMP = 3.0                    # amplitude of the Gaussian logits
TIE_SHARE = 0.005            # at most this share of the pixels may lie inside the tie band
EPS = 2.0 ** -24             # unit roundoff of float32


def windows_of(H, W, crop, stride):
    """(ny, nx, [(y, x), ...]) of the grid, restated from the header: n = max(L - c + s - 1, 0) // s + 1, origin min(i s, L - c)."""
    (ch, cw), (sh, sw) = crop, stride
    ny, nx = max(H - ch + sh - 1, 0) // sh + 1, max(W - cw + sw - 1, 0) // sw + 1
    return ny, nx, [(min(i * sh, H - ch), min(j * sw, W - cw)) for i in range(ny) for j in range(nx)]


def oracle(maps, H, W, crop, stride, dtype):
    """mmseg's slide_inference on given window outputs.  maps: CPU tensor [B, nWin, h, w, C] (NHWC per window, any float dtype; bf16
    values are widened exactly).  Every window is F.interpolate'd to the crop, added into a [B, C, H, W] accumulator at its origin, a
    count map gets + 1, then accumulator / count.  -> (mean [B, C, H, W] `dtype`, count [H, W] int64)."""
    B, nwin, h, w, C = maps.shape
    _, _, origins = windows_of(H, W, crop, stride)
    assert nwin == len(origins)
    acc = torch.zeros(B, C, H, W, dtype=dtype)
    cnt = torch.zeros(H, W, dtype=dtype)
    for k, (y, x) in enumerate(origins):
        z = F.interpolate(maps[:, k].to(dtype).permute(0, 3, 1, 2), size=tuple(crop), mode='bilinear', align_corners=False)
        acc[:, :, y:y + crop[0], x:x + crop[1]] += z
        cnt[y:y + crop[0], x:x + crop[1]] += 1
    return acc / cnt, cnt.to(torch.int64)


def make_maps(B, C, nwin, h, w, storage, seed=0, amp=AMP):
    """Seeded amp * randn window maps [B, nWin, h, w, C] (different data per image and window), rounded to `storage`."""
    g = torch.Generator().manual_seed(seed)
    return (amp * torch.randn(B, nwin, h, w, C, generator=g)).to(storage)


def atol_of(e32, n_max, M):
    """Tolerance of mean_out against the float64 oracle.  A pixel covered by n windows: at most 6 fp32 roundings per sample, n - 1
    additions on partial sums of at most n M, one division -> error <= (n^2 + 5 n + 1) 2^-24 M; 16 n covers that for every n <= 9
    (and is asked of the 16-fold case too, where the worst-case bound would be 337 units against these 256).  Floored at 4 x the
    float32 oracle's own error."""
    return max(4.0 * e32, 16.0 * n_max * EPS * M)


def tie_band(M64, atol):
    """bool [B, H, W]: pixels whose float64 top-2 margin of the mean logits is below 2 atol."""
    if M64.shape[1] < 2:
        return torch.zeros(M64.shape[0], *M64.shape[2:], dtype=torch.bool)
    top = M64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < 2.0 * atol


@functools.lru_cache(maxsize=None)
def case(C, H, W, crop, stride, hw, storage, B=2, seed=0):
    """The reference of one geometry, computed once, shared, never modified: dict(maps, M64, e32, n_max, M, atol, band)."""
    ny, nx, _ = windows_of(H, W, crop, stride)
    maps = make_maps(B, C, ny * nx, hw[0], hw[1], storage, seed)
    M64, cnt = oracle(maps, H, W, crop, stride, torch.float64)
    M32, _ = oracle(maps, H, W, crop, stride, torch.float32)
    e32 = (M32.double() - M64).abs().max().item()
    n_max, mag = int(cnt.max()), maps.double().abs().max().item()
    atol = atol_of(e32, n_max, mag)
    return dict(maps=maps, M64=M64, cnt=cnt, e32=e32, n_max=n_max, M=mag, atol=atol, band=tie_band(M64, atol))


def run_kernel(maps, C, H, W, crop, stride, target=None, ignore_label=255, want_pred=True, want_mean=True, ldl=None, mat_fill=0):
    """Call hip.slide_argmax_confmat on CPU window maps [B, nWin, h, w, C]; -> dict(mean [B, H, W, C] fp32, pred, mat, hist, flag) on
    the CPU.  ldl: row stride of the device rows (columns beyond C filled with a large value that must never be read as a class)."""
    from segmentation_factory_amd import hip
    B, nwin, h, w, _ = maps.shape
    r = maps.reshape(B * nwin * h * w, C)
    if ldl is not None and ldl != C:
        buf = torch.full((r.shape[0], ldl), 1e4, dtype=maps.dtype)
        buf[:, :C] = r
        r = buf.cuda()[:, :C]
    else:
        r = r.contiguous().cuda()
    mat = torch.full((C, C), mat_fill, dtype=torch.int64, device='cuda')
    hist = torch.full((C, C), mat_fill, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device='cuda') if want_pred else None
    mean = torch.full((B * H * W, C), -1.0, dtype=torch.float32, device='cuda') if want_mean else None
    tg = target.cuda() if target is not None else None
    hip.slide_argmax_confmat((r, h, w), B, C, H, W, crop, stride, tg, ignore_label, mat, hist, flag, pred_out=pred, mean_out=mean)
    torch.cuda.synchronize()
    return dict(mean=mean.cpu().view(B, H, W, C) if want_mean else None, pred=pred.cpu() if want_pred else None,
                mat=mat.cpu(), hist=hist.cpu(), flag=int(flag.item()))
