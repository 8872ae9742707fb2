"""Helpers of the multi-scale + flip (MSF) evaluation tests: the torch restatement of segf_msf_argmax_confmat (include/segfac.h)
and the standard case.  No test lives here."""
import functools

import torch
import torch.nn.functional as F

# (h, w, flip) of the standard case at H x W = 24 x 40
STANDARD_MAPS = (
    (6, 10, 0),      # ratio 4
    (5, 7, 1),       # non-integer ratio, odd width, mirrored
    (9, 15, 0),
    (12, 20, 1),
    (24, 40, 0),     # direct read
    (3, 5, 1),
    (42, 70, 0),     # h_k > H: downsampling without antialiasing
)
STANDARD_B, STANDARD_HW = 2, (24, 40)
TIE_MARGIN = 1e-4            # float64 top-2 margin of the summed probabilities below which a pixel's prediction is not compared
TIE_SHARE = 0.005            # at most this share of the pixels may be left out that way


def oracle(maps, flips, H, W, dtype):
    """Sum over the maps of softmax_c(F.interpolate(map, (H, W), bilinear, align_corners=False)), added in list order.
    maps: CPU tensors [B, h, w, C] (NHWC, any float dtype); flips[k]: map k belongs to the mirrored image.  -> [B, C, H, W] `dtype`."""
    S = None
    for m, f in zip(maps, flips):
        z = m.to(dtype)
        if f:
            z = z.flip(2)
        p = F.interpolate(z.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False).softmax(1)
        S = p if S is None else S + p
    return S


def make_maps(B, C, geoms, amp, storage, seed=0):
    """Seeded amp * randn maps [B, h, w, C], rounded to `storage` (so that the bf16 inputs are exact bf16 values)."""
    g = torch.Generator().manual_seed(seed)
    return [(amp * torch.randn(B, h, w, C, generator=g)).to(storage) for h, w, _ in geoms]


@functools.lru_cache(maxsize=None)
def standard_case(C, amp, storage, seed=0):
    """(maps, flips, S64, e32) of the standard case: the float64 oracle and the error of the float32 oracle against it (the
    yardstick of the probability tolerance; it comes from torch alone).  Cached: computed once, shared, never modified."""
    H, W = STANDARD_HW
    maps = make_maps(STANDARD_B, C, STANDARD_MAPS, amp, storage, seed)
    flips = [f for _, _, f in STANDARD_MAPS]
    S64 = oracle(maps, flips, H, W, torch.float64)
    e32 = (oracle(maps, flips, H, W, torch.float32).double() - S64).abs().max().item()
    return maps, flips, S64, e32


def prob_atol(e32):
    """Tolerance of prob_out against the float64 oracle: 8 x the float32 oracle's own error (room for a fast exp and another
    summation order inside the softmax), floored at 4e-6."""
    return max(8.0 * e32, 4e-6)


def tie_band(S64):
    """bool [B, H, W]: pixels whose float64 top-2 margin of the summed probabilities is below TIE_MARGIN."""
    if S64.shape[1] < 2:
        return torch.zeros(S64.shape[0], *S64.shape[2:], dtype=torch.bool)
    top = S64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < TIE_MARGIN


def make_target(B, H, W, C, ignore_label=255, bad_label=None, seed=1):
    """Labels in [0, C) with a band of ignore_label and, optionally, a few pixels of a bad label (outside [0, C), not ignored)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[:, :2] = ignore_label
    t[:, 5, ::3] = ignore_label
    if bad_label is not None:
        t[:, 7, 1:9] = bad_label
    return t


def counts(target, pred, C, ignore_label):
    """(mat, hist) int64 [C, C] of eval_count (csrc/eval_rows.h): torch bincount of (target, pred) over all pixels."""
    t, p = target.flatten(), pred.flatten()
    in_mat = (t >= 0) & (t < C)
    mat = torch.bincount(t[in_mat] * C + p[in_mat], minlength=C * C).view(C, C)
    k = in_mat & (t != ignore_label)
    hist = torch.bincount(t[k] * C + p[k], minlength=C * C).view(C, C)
    return mat, hist


def run_kernel(maps, flips, C, H, W, target=None, ignore_label=255, want_pred=True, want_prob=True, ldl=None):
    """Call hip.msf_argmax_confmat on CPU maps [B, h, w, C]; -> dict(prob [B, H, W, C] fp32, pred, mat, hist, flag) on the CPU.
    ldl: row stride of the device rows (columns beyond C filled with a large value that must never be read as a class)."""
    from segmentation_factory_amd import hip
    B = maps[0].shape[0]
    rows = []
    for m in maps:
        _, h, w, _ = m.shape
        r = m.reshape(B * h * w, C)
        if ldl is not None and ldl != C:
            buf = torch.full((B * h * w, ldl), 1e4, dtype=m.dtype)
            buf[:, :C] = r
            r = buf.cuda()[:, :C]
        else:
            r = r.contiguous().cuda()
        rows.append((r, h, w))
    mat = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device='cuda') if want_pred else None
    prob = torch.full((B * H * W, C), -1.0, dtype=torch.float32, device='cuda') if want_prob else None
    tg = target.cuda() if target is not None else None
    hip.msf_argmax_confmat(rows, flips, B, C, H, W, tg, ignore_label, mat, hist, flag, pred_out=pred, prob_out=prob)
    torch.cuda.synchronize()
    return dict(prob=prob.cpu().view(B, H, W, C) if want_prob else None, pred=pred.cpu() if want_pred else None,
                mat=mat.cpu(), hist=hist.cpu(), flag=int(flag.item()))
