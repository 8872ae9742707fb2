"""float64 restatement of the per-pixel losses of segmentation_factory_amd/losses.py (reference util/losses.py:9-66 on
F.interpolate(low, (H, W), bilinear, align_corners=False)): the per-pixel cross entropy, the reference's selection rule, the loss, and
the gradient with respect to the LOW-resolution logits, written out (no autograd), plus the input recipes the tests and
tools/make_pixel_loss_goldens.py share.

Selection can be made on an externally supplied CE map (the kernel's own fp32 map): the integers, kappa and the per-pixel coefficient
are then exact functions of that map, so the checks of the loss and of the gradient do not depend on which side of the decision value a
borderline pixel falls in fp32.  Ties at kappa share (n_min - n_gt) / (n_eq * n_min) each (include/segfac.h): torch.topk keeps arbitrary
members, the loss is the same."""
import math

import numpy as np
import torch

from loss_refs import taps

F64 = torch.float64
IGNORE = 255


def theta_of(thresh=0.7):
    """-torch.log(torch.tensor(thresh, dtype=torch.float)) of losses.py:49 as a Python float holding the fp32 value."""
    return float(-torch.log(torch.tensor(thresh, dtype=torch.float)))


# ---- the resize and its transpose, separable, float64 ---------------------------------------------------------------------------
def upsample(lo, H, W):
    """lo [B, h, w, C] float64 -> z [B, H, W, C]."""
    _, h, w, _ = lo.shape
    y0, y1, ly = taps(h, H)
    x0, x1, lx = taps(w, W)
    rows = lo[:, y0] * (1 - ly)[None, :, None, None] + lo[:, y1] * ly[None, :, None, None]
    return rows[:, :, x0] * (1 - lx)[None, None, :, None] + rows[:, :, x1] * lx[None, None, :, None]


def upsample_T(dz, h, w):
    """dz [B, H, W, C] -> d lo [B, h, w, C]: the transposed resize."""
    B, H, W, C = dz.shape
    y0, y1, ly = taps(h, H)
    x0, x1, lx = taps(w, W)
    tmp = torch.zeros(B, H, w, C, dtype=F64)
    tmp.index_add_(2, x0, dz * (1 - lx)[None, None, :, None])
    tmp.index_add_(2, x1, dz * lx[None, None, :, None])
    out = torch.zeros(B, h, w, C, dtype=F64)
    out.index_add_(1, y0, tmp * (1 - ly)[None, :, None, None])
    out.index_add_(1, y1, tmp * ly[None, :, None, None])
    return out


# ---- per-pixel CE ---------------------------------------------------------------------------------------------------------------
def ce(lo, t, cw=None, ignore=IGNORE):
    """(ce [B, H, W], p [B, H, W, C], valid [B, H, W], wt [B, H, W]): ce = w[t] (logsumexp z - z_t), +0 where t == ignore."""
    lo = lo.to(F64)
    H, W = t.shape[-2:]
    C = lo.shape[-1]
    z = upsample(lo, H, W)
    lse = torch.logsumexp(z, dim=-1)
    valid = (t != ignore) & (t >= 0) & (t < C)
    tc = torch.where(valid, t, torch.zeros_like(t))
    zt = z.gather(-1, tc[..., None])[..., 0]
    wt = torch.ones_like(lse) if cw is None else cw.to(F64)[tc]
    c = torch.where(valid, (wt * (lse - zt)).clamp_min(0.0), torch.zeros_like(lse))
    return c, torch.softmax(z, dim=-1), valid, wt


# ---- selection, loss, coefficient -----------------------------------------------------------------------------------------------
def ohem(cmap, t, theta, ignore=IGNORE):
    """The reference's rule on a CE map (float64, or the kernel's fp32 map: comparisons are then exact).  Returns a dict with the
    integers, kappa (the decision value), loss (float64; NaN for an empty selection) and coef [B, H, W] = d loss / d ce."""
    c = cmap.to(F64)
    flat = c.reshape(-1)
    n_valid = int((t != ignore).sum())
    n_min = n_valid // 16
    hard = flat > theta
    n_hard = int(hard.sum())
    out = {'n_valid': n_valid, 'n_min': n_min, 'n_hard': n_hard}
    if n_hard >= n_min:
        out.update(used_topk=0, kappa=theta, n_gt=n_hard, n_eq=0, n_sel=n_hard)
        out['loss'] = flat[hard].sum() / n_hard if n_hard else torch.tensor(math.nan, dtype=F64)
        coef = hard.to(F64) / n_hard if n_hard else torch.zeros_like(flat)
    else:
        kappa = torch.topk(flat, n_min).values[-1]
        gt, eq = flat > kappa, flat == kappa
        n_gt, n_eq = int(gt.sum()), int(eq.sum())
        out.update(used_topk=1, kappa=float(kappa), n_gt=n_gt, n_eq=n_eq, n_sel=n_min)
        out['loss'] = (flat[gt].sum() + (n_min - n_gt) * kappa) / n_min
        coef = gt.to(F64) / n_min + eq.to(F64) * ((n_min - n_gt) / (n_eq * n_min))      # the tie-sharing rule
    out['coef'] = coef.reshape(c.shape)
    return out


def focal(cmap, alpha, gamma, size_average=True):
    """{'loss', 'coef'}: f = alpha (1 - pt)^gamma ce over ALL pixels; coef = d loss / d ce."""
    c = cmap.to(F64)
    n = c.numel() if size_average else 1
    q = -torch.expm1(-c)                       # 1 - pt
    pt = 1 - q
    f = alpha * q ** gamma * c if gamma else alpha * c
    slope = q ** gamma if gamma else torch.ones_like(c)
    if gamma:
        extra = gamma * torch.where(c > 0, q.clamp_min(1e-300) ** (gamma - 1), torch.zeros_like(c)) * pt * c
        slope = slope + torch.where(c > 0, extra, torch.zeros_like(c))
    return {'loss': f.sum() / n, 'coef': alpha * slope / n}


def grad_low(lo, t, coef, cw=None, go=1.0, ignore=IGNORE):
    """d loss / d lo [B, h, w, C]: go * coef * w[t] * (softmax - onehot) on the valid pixels, through the transposed resize."""
    _, p, valid, wt = ce(lo, t, cw, ignore)
    C = lo.shape[-1]
    tc = torch.where(valid, t, torch.zeros_like(t))
    onehot = torch.nn.functional.one_hot(tc, C).to(F64)
    dz = (go * coef.to(F64) * wt * valid.to(F64))[..., None] * (p - onehot)
    return upsample_T(dz, lo.shape[1], lo.shape[2])


def ohem_statement(lo, t, theta, cw=None, go=1.0, ignore=IGNORE, select_on=None):
    """(loss, d lo, info): the whole OHEM loss; select_on = a CE map to select on instead of the float64 one."""
    c = ce(lo, t, cw, ignore)[0]
    sel = ohem(c if select_on is None else select_on, t, theta, ignore)
    return sel['loss'], grad_low(lo, t, sel['coef'], cw, go, ignore), sel


def focal_statement(lo, t, alpha, gamma, size_average=True, go=1.0, ignore=IGNORE):
    c = ce(lo, t, None, ignore)[0]
    f = focal(c, alpha, gamma, size_average)
    return f['loss'], grad_low(lo, t, f['coef'], None, go, ignore), f


# ---- input recipes (B, C, h, w, H, W) -------------------------------------------------------------------------------------------
def ignore_pattern(t, g, rows=2, frac=0.02, ignore=IGNORE):
    t = t.clone()
    t[:, :rows] = ignore
    t[torch.rand(t.shape, generator=g) < frac] = ignore
    return t


def plain_inputs(geom, seed):
    """Threshold branch: randn logits, uniform labels, rows 0-1 and 2 % of the pixels ignored."""
    B, C, h, w, H, W = geom
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(B, h, w, C, generator=g)
    t = torch.randint(0, C, (B, H, W), generator=g)
    return lo, ignore_pattern(t, g)


def confident_inputs(geom, seed, raise_by=6.0):
    """Top-k branch: per image one class whose low-res logit is raised; labels equal it except for 1 % random other labels."""
    B, C, h, w, H, W = geom
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(B, h, w, C, generator=g)
    kb = torch.randint(0, C, (B,), generator=g)
    lo[torch.arange(B), :, :, kb] += raise_by
    t = kb[:, None, None].expand(B, H, W).clone()
    other = torch.rand(B, H, W, generator=g) < 0.01
    t = torch.where(other, (t + torch.randint(1, C, (B, H, W), generator=g)) % C, t)
    return lo, ignore_pattern(t, g)


def random_weights(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.5 + 2.5 * torch.rand(C, generator=g)


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pixel_loss_cases.npz')


def load_golden():
    """{case name: {field: array}} of tests/golden/pixel_loss_cases.npz (tools/make_pixel_loss_goldens.py)."""
    g = np.load(golden_path(), allow_pickle=False)
    cases = {}
    for key in g.files:
        name, field = key.split('/', 1)
        cases.setdefault(name, {})[field] = g[key]
    return cases
