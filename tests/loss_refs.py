"""Float64 statement of the fused bilinear upsample + CrossEntropy + Dice loss (csrc/loss.hip, csrc/loss_band.hip), its two reference
statements (plain fp32; float64 with the documented bf16 roundings of the matrix-pipe paths), the condition scales that the bounds of
tests/test_loss_float64.py are built from, the wrong computations (MUTANTS) the comparator must reject, and the case tables.
Importable without a GPU.

The formulas are those of the header comment of csrc/loss.hip and of include/segfac.h, not a transcription of the kernels:
    z = bilinear(low-res logits), align_corners=False          p = softmax_c z            valid = label != ignore_index
    I_bc = sum_valid p_c [t = c]    P_bc = sum_valid p_c    T_bc = sum_valid [t = c]       (per image b)
    ce_sum_b = sum_valid cw[t] (log sum_c exp z - z_t)      w_sum_b = sum_valid cw[t]       n_valid_b = sum_valid 1
    ce = sum_b ce_sum / sum_b w_sum       dice_loss = 1 - mean_bc (2 I + eps) / (sets + eps),   sets = P + T, (sets == 0 -> 2 I), eps = 1e-6
    loss = {ce + dice_loss, ce, dice_loss}
    gI = -2 nbc / (sets + eps)     gP = nbc (2 I + eps) / (sets + eps)^2     nbc = 1 / (B C), both 0 where sets == 0
    G = gP + [c == t] gI           wce = cw[t] / sum_b w_sum
    dz = go ( p_c (G_c - <G, p>) + wce (p_c - [c == t]) )  on valid pixels;     d(low-res logits) = transposed bilinear resize of dz
The logits are given ALREADY ROUNDED to the storage type, as float64 (`norm_refs.to_storage`).

Condition scale S of a gradient element: the same transposed resize of the absolute values of the parts that are formed separately,
    Sz = go p_c |wce - <G, p>| + go p_c |gP_c| + [c == t] (|go p_t gI_t| + go wce)
of a statistic: the float64 sum of the absolute values of its terms (I, P, w_sum: the value; ce_sum: sum cw[t] (1 + |z_t - max| +
|log-sum - z_t|): the difference is formed from z_t - max and from the log of a rounded sum >= 1, which carries an absolute error
2^-24 whatever is left of the difference); of a loss value: those scales carried through the quotients (`loss_scales`).

Bound of every comparison (norm_refs.compare, group = the whole tensor of a case, floor 0):
    |got - ref64| <= half_ulp_T(ref64) + MARGIN * K * u * S,        MARGIN = 4 (norm_refs' margin of elementwise outputs)
    u = 2^-24 on the fp32-arithmetic paths, 2^-9 on the bf16-tile paths (the band forward's P; every bf16-storage ratio-4 backward)
    K = the largest |statement - ref64| / (u S) over every element of every case of the tables below, of `stmt32` (u = 2^-24) and of
        `stmt_bf16tile` (u = 2^-9): the references' OWN error.  The values are cached here and re-derived by
        tests/test_loss_float64.py::test_cached_K_is_what_the_statements_measure (a CPU test).

Measured K (torch on the CPU, every case of cpu_cases() and gpu_cases(), both storage types; the cached K32 / KBF are these, rounded up):
    stmt32, power-of-two ratios:  grad 85.1  I 126.1  P 58.8  ce_sum 2.09  w_sum 4.47  loss 15.1  log-sum 4.75
    stmt32, other ratios:         grad 37.1  I 12.5   P 4.78  ce_sum 1.04  w_sum 1.10  loss 14.2
    stmt_bf16tile:                grad 4.98  P 2.75
K is kept per output and per geometry class (`geom_class`); each is at most the single largest value over the table.

Terms that no relative bound carries are DERIVED where they arise and added to the allowed error: `under` (exponentials below 2^-126
are flushed to zero), `wobble` (fp32 tap weights of the non-dyadic ratios), the stabiliser in the log-sum buffer (`lse_entry`); the
terms of single kernel paths are in tests/test_loss_float64.py (`_derived`).
"""
import math

import torch
import torch.nn.functional as F

import exact_inputs as X
from norm_refs import BF, F32, F64, U24, Verdict, check, compare, half_ulp, seed_of, to_storage   # noqa: F401  (one comparator)

U9 = 2.0 ** -9                         # half a unit in the last place of a bf16 value in [1, 2)
MARGIN = 4.0
EPS = 1e-6
IGNORE = 255
LN2 = math.log(2.0)
WEIGHT_ROUNDINGS = 8                   # see `statement`: roundings on the way to a tap weight of a non-dyadic ratio
FLUSH = 2.0 ** -126                    # smallest normal fp32 / bf16 value: an exponential below it may be flushed to 0

# The cached K: outputs -> the largest |stmt - ref64| / (u S) (see the module docstring).  Rounded up to two digits from the measured
# values; test_cached_K_is_what_the_statements_measure asserts measured <= cached <= 2 * measured.
K32 = {'pow2': {'grad': 86.0, 'I': 127.0, 'P': 59.0, 'ce_sum': 2.1, 'w_sum': 4.5, 'loss': 15.2, 'lse': 4.8},
       'generic': {'grad': 37.5, 'I': 12.7, 'P': 4.8, 'ce_sum': 1.05, 'w_sum': 1.11, 'loss': 14.3, 'lse': 67.2}}
KBF = {'grad': 5.0, 'P': 2.75}


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def taps(n_in, n_out, mut=None):
    """(i0, i1, l) float64 / int64 [n_out]: source taps and the weight of i1, F.interpolate(mode='bilinear', align_corners=False).
    mut: 'align_corners', 'no_half_pixel', 'zero_pad' (i0 / i1 may then lie outside [0, n_in): the caller drops those taps)."""
    d = torch.arange(n_out, dtype=F64)
    if mut == 'align_corners':
        src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    elif mut == 'no_half_pixel':
        src = d * (n_in / n_out)
    else:
        src = (d + 0.5) * (n_in / n_out) - 0.5
        if mut != 'zero_pad':
            src = src.clamp_min(0.0)
    i0 = torch.floor(src).long()
    l = src - i0
    i1 = i0 + 1
    if mut != 'zero_pad':
        i1 = i1.clamp_max(n_in - 1)
    return i0, i1, l


_OPS = {}


def resize_op(h, w, H, W, mut=None):
    """The upsample as a dense float64 matrix A [H * W][h * w]: z = A @ low, d low = A^T @ dz.  Exact for the power-of-two ratios (the
    weights are dyadic); for the others the weights are the float64 ones."""
    key = (h, w, H, W, mut)
    if key in _OPS:
        return _OPS[key]
    rm = mut if mut in ('align_corners', 'no_half_pixel', 'zero_pad') else None
    y0, y1, ly = taps(h, H, rm)
    x0, x1, lx = taps(w, W, rm)
    LY, LX = ly[:, None].expand(H, W), lx[None, :].expand(H, W)
    if mut == 'lylx_swapped':                            # the row fraction weighs the columns and the other way round
        ly2, lx2 = taps(h, W, None)[2], taps(w, H, None)[2]
        LY, LX = ly2[None, :].expand(H, W), lx2[:, None].expand(H, W)
    A = torch.zeros(H * W, h * w, dtype=F64)
    Pm = torch.zeros(H * W, h * w, dtype=F64)             # 1 on the (up to four) taps of a pixel, the ones of weight zero included
    rows = torch.arange(H * W)
    for yy, wy in ((y0, 1 - LY), (y1, LY)):
        for xx, wx in ((x0, 1 - LX), (x1, LX)):
            ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
            col = (yy.clamp(0, h - 1)[:, None] * w + xx.clamp(0, w - 1)[None, :]).reshape(-1)
            A.index_put_((rows, col), (wy * wx * ok).reshape(-1), accumulate=True)
            Pm[rows, col] = 1.0
    if mut is None:                                       # a source coordinate on a whole number: fp32 may land just below it
        ys = [(y0, torch.ones(H, dtype=torch.bool)), (y1, torch.ones(H, dtype=torch.bool)), ((y0 - 1).clamp_min(0), ly < 1e-5)]
        xs = [(x0, torch.ones(W, dtype=torch.bool)), (x1, torch.ones(W, dtype=torch.bool)), ((x0 - 1).clamp_min(0), lx < 1e-5)]
        for yy, oky in ys:
            for xx, okx in xs:
                sel = (oky[:, None] & okx[None, :]).reshape(-1)
                col = (yy[:, None] * w + xx[None, :]).reshape(-1)
                Pm[rows[sel], col[sel]] = 1.0
    if len(_OPS) > 64:
        _OPS.clear()
    _OPS[key] = A
    _OPS[key + ('taps',)] = Pm
    return A


def tap_pattern(h, w, H, W):
    resize_op(h, w, H, W)
    return _OPS[(h, w, H, W, None, 'taps')]


def dyadic(h, w, H, W):
    """Are the tap weights exact in every format (ratios 1, 2, 4, 8, 16 in both directions)?"""
    return H % h == 0 and W % w == 0 and (H // h) & (H // h - 1) == 0 and (W // w) & (W // w - 1) == 0


def nt_bucket(C):
    """(NT, FULL0) of the ratio-4 matrix-pipe kernels (LS_NT_DISPATCH of csrc/loss.hip; loss_band_*_launch)."""
    nt = (C + 15) // 16
    NT = 2 if nt <= 2 else 4 if nt <= 4 else 10 if nt <= 10 else 12
    return NT, C >= {2: 32, 4: 64, 10: 128, 12: 128}[NT]


def bf(t):
    return t.to(F32).to(BF).double()


# ---- the statement -------------------------------------------------------------------------------------------------------------------
MUTANTS = ('no_gP', 'gI_all_classes', 'nbc_1_over_B', 'eps_10x', 'ignored_in_P', 'ce_by_n_valid', 'cw_at_pred', 'align_corners',
           'no_half_pixel', 'zero_pad', 'lylx_swapped', 'label_plus1', 'last_tile_dropped', 'dup_last_class', 'go_not_on_dice',
           'stats_prev_image')
# `no_sets0_rule` computes the same function: sets = P + T == 0 needs an image without valid pixels (p > 0 in float64 for every
# logit the tables hold) or p_c == 0 on all of them, and then I == 0 too: (2 I + eps) / (sets + eps) = eps / eps = 1 with and without
# the rule, and gP = nbc / eps multiplies p_c of no pixel (or p_c == 0).  test_sets0_rule_is_not_observable pins this.
EQUIVALENT_MUTANTS = ('no_sets0_rule',)


def statement(lo, t, cw=None, go=1.0, dice=True, mut=None, rnd=None):
    """lo float64 [B][C][h][w] (rounded to the storage type), t int64 [B][H][W], cw fp32 / float64 [C] or None.
    rnd='bf16tile': the documented roundings of the bf16 matrix-pipe paths (see stmt_bf16tile).
    -> dict(loss [3], I, P, T [B][C], ce_sum, w_sum, n_valid [B], grad [B * h * w][C], lse [B][(h + 1)(w + 1)][16] for ratio 4, and the
    scales S_grad, S_I, S_P, S_ce_sum, S_w_sum, S_loss (see loss_scales))."""
    lo = lo.double()
    B, C, h, w = lo.shape
    H, W = t.shape[1:]
    A = resize_op(h, w, H, W, mut)
    low = lo.permute(0, 2, 3, 1).reshape(B, h * w, C)
    z = A @ low                                                        # [B][HW][C]
    tt = t.reshape(B, -1)
    valid = tt != IGNORE
    vf = valid.double()
    tl = torch.where(valid, tt, torch.zeros_like(tt))
    if mut == 'label_plus1':
        tl = (tl - 1) % C
    zs = z
    if mut == 'last_tile_dropped':
        zs = z.masked_fill(torch.arange(C) >= 16 * (nt_bucket(C)[0] - 1), -math.inf)
    m = zs.amax(-1, keepdim=True)
    e = torch.exp(zs - m)
    s = e.sum(-1, keepdim=True)
    if mut == 'dup_last_class':
        s = s + e[..., C - 1:]
    p = e / s
    lse = (m + torch.log(s))[..., 0]
    oh = F.one_hot(tl, C).double() * vf[..., None]
    pv = p * vf[..., None]
    I = (pv * oh).sum(1)
    if rnd == 'bf16tile':                                              # P on the matrix pipe: A row = ok / sum, B = the exp tile, both bf16
        P = (bf(e) * bf(vf[..., None] / s)).sum(1)
    else:
        P = (p if mut == 'ignored_in_P' else pv).sum(1)
    T = oh.sum(1)
    cwv = torch.ones(C, dtype=F64) if cw is None else cw.double()
    wt = (cwv[z.argmax(-1)] if mut == 'cw_at_pred' else cwv[tl]) * vf
    nll = lse - z.gather(-1, tl[..., None])[..., 0]
    ce_sum, w_sum, n_valid = (wt * nll).sum(1), wt.sum(1), vf.sum(1)
    Wtot = n_valid.sum() if mut == 'ce_by_n_valid' else w_sum.sum()
    ce = ce_sum.sum() / Wtot
    eps = 10 * EPS if mut == 'eps_10x' else EPS
    sets = P + T
    zero = (sets == 0) & (mut != 'no_sets0_rule')
    den = torch.where(zero, 2 * I, sets) + eps
    d = (2 * I + eps) / den
    nbc = 1.0 / B if mut == 'nbc_1_over_B' else 1.0 / (B * C)
    dl = 1 - nbc * d.sum() if dice else torch.zeros((), dtype=F64)
    loss = torch.stack([ce + dl, ce, dl])
    on = 1.0 if dice else 0.0
    gI = torch.where(zero, torch.zeros_like(sets), -2 * nbc / (sets + eps)) * on
    gP = torch.where(zero, torch.zeros_like(sets), nbc * (2 * I + eps) / (sets + eps) ** 2) * on
    if mut == 'stats_prev_image':
        gI, gP = gI.roll(1, 0), gP.roll(1, 0)
    if mut == 'no_gP':
        gP = torch.zeros_like(gP)
    G = gP[:, None, :] + (gI[:, None, :] if mut == 'gI_all_classes' else oh * gI[:, None, :])
    dot = (G * p).sum(-1, keepdim=True)
    wce = torch.where(valid, wt / Wtot, torch.zeros_like(wt))[..., None]      # an ignored pixel has no CE term (not 0 * inf)
    go = float(go)
    go_d = 1.0 if mut == 'go_not_on_dice' else go
    v3 = vf[..., None]
    if rnd == 'bf16tile':
        # scatter on the matrix pipe: per tap, sum_pixels bf16(weight * k) * bf16(p_c) + gP_c * sum_pixels bf16(weight * go) * bf16(p_c);
        # the label-class terms stay fp32
        pb = bf(p)
        k1 = go * (wce - dot) * v3                                    # [B][HW][1]
        A1 = bf(A[None] * k1)                                         # [B][HW][hw]
        A2 = bf(A * go)[None] * v3
        grad = A1.transpose(1, 2) @ pb + gP[:, None, :] * (A2.transpose(1, 2) @ pb)
        grad = grad + A.T @ (oh * (go * p * gI[:, None, :] - go * wce))
    else:
        dz = (go_d * p * (G - dot) + go * wce * (p - oh)) * v3
        grad = A.T @ dz
    Sz = (go * p * (wce - dot).abs() + go * p * gP[:, None, :].abs() + oh * ((go * p * gI[:, None, :]).abs() + go * wce)) * v3
    Sz = torch.where(v3 > 0, Sz, torch.zeros_like(Sz))                 # (an all-ignored batch: wce is NaN-free above, keep S so)
    # what no relative bound carries (see `entries`): the flush of exp below 2^-126, and the cancellation in log-sum - z_t
    m1 = m[..., 0]
    mb = torch.where(A > 0, low.amax(-1)[:, None, :], torch.full((), -math.inf, dtype=F64)).amax(-1)      # largest logit of the pixel's taps
    zt = z.gather(-1, tl[..., None])[..., 0]
    coef = go * ((wce - dot).abs() + gP[:, None, :].abs()) * v3
    under = {}
    for name, top in (('exact', m1), ('cell', mb)):
        eta = (FLUSH * torch.exp(top - lse)).clamp_max(FLUSH / 1e-30)
        under[name] = dict(grad=(A.T @ (eta[..., None] * coef)).reshape(B * h * w, C), P=(eta * vf).sum(1)[:, None].expand(B, C),
                           I=(oh * eta[..., None]).sum(1))
    # non-dyadic ratios: a tap weight formed in fp32 (src = scale (dst + 1/2) - 1/2, the fraction, its complement, the product of two)
    # carries an ABSOLUTE error <= WEIGHT_ROUNDINGS 2^-24 max(h, w), also where the exact weight is 0.  First order: the gradient moves by
    # that times sum |dz| over the pixels of the tap; a logit by that times the spread of the class over the pixel's taps, a
    # probability by twice the largest such spread (relative).
    wob = None
    dzabs = ((go * p * (G - dot) + go * wce * (p - oh)) * v3).abs()
    if not dyadic(h, w, H, W) and mut is None and rnd is None:
        dw = WEIGHT_ROUNDINGS * U24 * max(h, w)
        Pm = tap_pattern(h, w, H, W)
        lowm = torch.where(Pm[None, :, :, None] > 0, low[:, None, :, :], torch.full((), math.nan, dtype=F64))     # [B][HW][hw][C]
        spread = (torch.nan_to_num(lowm, nan=-math.inf).amax(2) - torch.nan_to_num(lowm, nan=math.inf).amin(2)).amax(-1)        # [B][HW]
        rel = 2 * dw * spread
        wob = dict(grad=(dw * (Pm.T @ dzabs) + A.T @ (rel[..., None] * Sz)).reshape(B * h * w, C), P=(rel[..., None] * pv).sum(1),
                   I=(rel[..., None] * pv * oh).sum(1), ce_sum=(wt * dw * spread).sum(1))
    out = dict(wobble=wob, stage_abs=(A.T @ dzabs).reshape(B * h * w, C), loss=loss, I=I, P=P, T=T, ce_sum=ce_sum, w_sum=w_sum, n_valid=n_valid, grad=grad.reshape(B * h * w, C),
               S_grad=(A.T @ Sz).reshape(B * h * w, C), S_I=I, S_P=P, S_ce_sum=(wt * (1 + nll.abs() + (zt - m1).abs())).sum(1), S_w_sum=w_sum,
               D_ce_cell=(wt * (mb - m1)).sum(1), D_ce_abs=(wt * (lse.abs() + zt.abs())).sum(1), under=under,
               lse=lse_layout(-lse.reshape(B, H, W) / LN2, h, w) if (H, W) == (4 * h, 4 * w) else None, lse_full=lse.reshape(B, H, W),
               lse_bound=lse_layout(mb.abs().reshape(B, H, W) / LN2, h, w) if (H, W) == (4 * h, 4 * w) else None)
    out.update(loss_scales(out, B, C, dice, eps))
    return out


def loss_scales(o, B, C, dice, eps=EPS):
    """Scales of loss = {total, ce, dice_loss}, split into the part that the fp32 sums carry (S_loss) and the part that P carries
    (S_loss_P: it takes u = 2^-9 where P comes off the bf16 tiles).
    ce = ce_sum / w: a quotient of two sums -> S_ce_sum / w + |ce| (the scale of w is w); plus |ce| for the rounding of the quotient.
    d_bc = (2 I + eps) / (sets + eps): 2 S_I / den + d S_P / den; dice_loss = 1 - mean d: the mean of those, + mean d for the roundings
    of the quotients and of their sum, + 1 for the subtraction from 1."""
    Wt = o['w_sum'].sum()
    ce_s = o['S_ce_sum'].sum() / Wt + 2 * o['loss'][1].abs()
    sets = o['P'] + o['T']
    den = torch.where(sets == 0, 2 * o['I'], sets) + eps
    d = (2 * o['I'] + eps) / den
    nbc = 1.0 / (B * C)
    dl_s = (1 + nbc * (2 * o['S_I'] / den + d).sum()) if dice else torch.zeros((), dtype=F64)
    dl_p = nbc * (d * o['S_P'] / den).sum() if dice else torch.zeros((), dtype=F64)
    z = torch.zeros((), dtype=F64)
    return dict(S_loss=torch.stack([ce_s + dl_s, ce_s, dl_s]), S_loss_P=torch.stack([dl_p, z, dl_p]))


def lse_layout(nl, h, w):
    """Per-pixel values [B][4h][4w] -> the hand-over buffer's cell layout [B][(h + 1)(w + 1)][16]: pixel (y, x) lives in cell
    ((y + 2) // 4, (x + 2) // 4), slot ((y + 2) % 4) * 4 + (x + 2) % 4.  Slots of pixels outside the image hold NaN here."""
    B, H, W = nl.shape
    cell, slot = lse_index(h, w)
    out = torch.full((B, (h + 1) * (w + 1), 16), math.nan, dtype=nl.dtype)
    out[:, cell, slot] = nl
    return out


def lse_index(h, w):
    ys, xs = torch.arange(4 * h), torch.arange(4 * w)
    cell = ((ys + 2) // 4)[:, None] * (w + 1) + ((xs + 2) // 4)[None, :]
    slot = (((ys + 2) % 4) * 4)[:, None] + ((xs + 2) % 4)[None, :]
    return cell, slot


def lse_unlayout(buf, h, w):
    """The inverse: [B][(h + 1)(w + 1)][16] -> [B][4h][4w]."""
    cell, slot = lse_index(h, w)
    return buf[:, cell, slot]


# ---- the two reference statements ----------------------------------------------------------------------------------------------------
def stmt32(lo, t, cw=None, go=1.0, dice=True):
    """Plain fp32 on the CPU: oracle.loss.criterion_closed_form on F.interpolate, with autograd; the statistics (which the oracle does
    not expose) as torch fp32 sums of fp32 softmax terms.  -> dict(loss, grad, I, P, ce_sum, w_sum, lse_full)."""
    from oracle import loss as OL
    B, C, h, w = lo.shape
    H, W = t.shape[1:]
    lr = lo.float().clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode='bilinear', align_corners=False)
    cw32 = None if cw is None else cw.float()
    total = OL.criterion_closed_form(up, t, cw32, num_classes=C, dice=dice, ignore_index=IGNORE)
    (float(go) * total).backward()
    u = up.detach()
    ce = F.cross_entropy(u, t, ignore_index=IGNORE, weight=cw32)
    valid = (t != IGNORE)
    tl = torch.where(valid, t, torch.zeros_like(t))
    p = F.softmax(u, 1)
    oh = F.one_hot(tl, C).permute(0, 3, 1, 2).float() * valid[:, None].float()
    wt = (torch.ones(C) if cw32 is None else cw32)[tl] * valid.float()
    lse = torch.logsumexp(u, 1)
    nll = lse - u.gather(1, tl[:, None])[:, 0]
    dl = total.detach() - ce if dice else torch.zeros(())
    return dict(loss=torch.stack([total.detach(), ce, dl]), grad=lr.grad.permute(0, 2, 3, 1).reshape(B * h * w, C),
                I=(p * oh).sum((2, 3)), P=(p * valid[:, None].float()).sum((2, 3)), ce_sum=(wt * nll).sum((1, 2)), w_sum=wt.sum((1, 2)),
                lse_full=lse)


def stmt_bf16tile(lo, t, cw=None, go=1.0, dice=True):
    """The float64 statement with the roundings that the bf16 paths document (csrc/loss_band.hip, header): exponentials and the
    per-pixel 1 / sum rounded to bf16 before the P sums of the forward; probabilities rounded to bf16 before the scatter of the
    backward; the per-pixel coefficient go (wce - <G, p>) times the tap weight (and go times the tap weight of the class-dependent Dice
    part) rounded to bf16; I, ce_sum, the label-class terms and the log-sum buffer stay fp32 (float64 here)."""
    return statement(lo, t, cw, go, dice, rnd='bf16tile')


# ---- bounds and judges ---------------------------------------------------------------------------------------------------------------
def geom_class(c):
    """K is kept per geometry class: the dyadic tap weights of the power-of-two ratios are exact in every format, the others are not
    (F.interpolate forms them in fp32).  Each is at most the one K over the whole table that the bound is defined with."""
    return 'generic' if c['path'] == 'generic' else 'pow2'


def entries(ref, dtype, geom='pow2', tile_fwd=False, tile_bwd=False, bound='cell', derived=None):
    """{output: dict(ref, e, scale, store, extra)} for norm_refs.compare.  tile_fwd: P comes off bf16 tiles; tile_bwd: so does the
    gradient.  bound: which maximum the exponentials are taken against ('exact': the pixel's; 'cell': the largest logit of the
    pixel's four taps, the batched kernels' wave-uniform bound).
    `extra`, DERIVED for every case: an exponential below 2^-126 is flushed to zero in fp32 and bf16, which float64 does not do, so a
    probability carries the ABSOLUTE error 2^-126 exp(bound - log-sum) besides its relative one; the term is that error carried
    through the same sums (`under` of the statement).  It is below 1e-8 of a coefficient by the kernels' retry threshold (sum > 1e-30).
    derived: {output: further absolute term} of a case (listed in the test module)."""
    k32 = K32[geom]
    kg, ug = (KBF['grad'], U9) if tile_bwd else (k32['grad'], U24)
    kp, up = (KBF['P'], U9) if tile_fwd else (k32['P'], U24)
    un = ref['under'][bound]
    e_loss = k32['loss'] * U24 * (ref['S_loss'] + ref['S_loss_P']) + (kp * up * ref['S_loss_P'] if tile_fwd else 0.0)
    en = dict(grad=dict(ref=ref['grad'], e=kg * ug * ref['S_grad'], scale=ref['S_grad'], store=dtype, extra=MARGIN * un['grad']),
              I=dict(ref=ref['I'], e=k32['I'] * U24 * ref['S_I'], scale=ref['S_I'], store=F32, extra=MARGIN * un['I']),
              P=dict(ref=ref['P'], e=kp * up * ref['S_P'], scale=ref['S_P'], store=F32, extra=MARGIN * un['P']),
              ce_sum=dict(ref=ref['ce_sum'], e=k32['ce_sum'] * U24 * ref['S_ce_sum'], scale=ref['S_ce_sum'], store=F32, extra=None),
              w_sum=dict(ref=ref['w_sum'], e=k32['w_sum'] * U24 * ref['S_w_sum'], scale=ref['S_w_sum'], store=F32, extra=None),
              loss=dict(ref=ref['loss'], e=e_loss, scale=ref['S_loss'] + ref['S_loss_P'], store=F32, extra=None))
    derived = dict(derived or {})
    if ref['wobble'] is not None:                        # non-dyadic ratios, DERIVED at `statement`: the fp32 tap weights
        for name, v in ref['wobble'].items():
            derived[name] = MARGIN * v + derived.get(name, 0.0)
        derived['loss'] = MARGIN * ref['wobble']['ce_sum'].sum() / ref['w_sum'].sum() + derived.get('loss', 0.0)
    for name, extra in derived.items():
        en[name]['extra'] = extra if en[name]['extra'] is None else en[name]['extra'] + extra
    return en


def judge(en, got, what, only=None):
    """{output: Verdict} of the outputs of `got` that have an entry: |got - ref64| <= half_ulp + MARGIN * e (+ derived)."""
    out = {}
    for name, d in en.items():
        if (only is None or name in only) and got.get(name) is not None:
            out[name] = compare(got[name], d['ref'], d['e'], d['scale'], d['store'], 'elementwise', f'{what} {name}', margin=MARGIN, floor=0.0,
                                extra=d.get('extra'))
    return out


def lse_entry(ref):
    """The log-sum buffer (exp2 domain): u = 2^-24, scale max(1, |ref|); slots outside the image are not compared.
    DERIVED `extra`: the buffer is formed as -(bound log2 e + log2 sum_c 2^(z_c log2 e - bound log2 e)), bound = the largest logit of the
    pixel's four taps: the product and the sum each round a value of the size of the bound, 2 * 2^-24 |bound| log2 e, whatever
    is left of it in the result (a spike in a neighbouring tap; a single class, where the result is the logit itself)."""
    r = ref['lse']
    keep = ~torch.isnan(r)
    r0 = torch.where(keep, r, torch.zeros_like(r))
    sc = r0.abs().clamp_min(1.0)
    return dict(ref=r0, e=K32['pow2']['lse'] * U24 * sc, scale=sc, keep=keep,
                extra=2 * U24 * torch.where(keep, ref['lse_bound'], torch.zeros_like(r)))


def measure_K(cases):
    """(K32, KBF) in the layout of the cached tables: the largest (|stmt - ref64| - flush term) / (u S) of stmt32 over `cases` in
    both storage types, and of stmt_bf16tile over the bf16 ratio-4 cases."""
    def worst(st, ref, name, S, u, under=None):
        e = (st.double().reshape(ref.shape) - ref).abs()
        if under is not None:
            e = (e - under).clamp_min(0)
        r = torch.where(S > 0, e / (u * S), torch.where(e > 0, torch.full_like(e, math.inf), torch.zeros_like(e)))
        r = torch.where(torch.isnan(ref) & torch.isnan(st.double().reshape(ref.shape)), torch.zeros_like(r), r)
        return r.max().item()
    k32 = {gm: dict.fromkeys(K32['pow2'], 0.0) for gm in K32}
    kbf = dict.fromkeys(KBF, 0.0)
    for c in cases:
        for dt in dtypes_of(c):
            inp = inputs(c, dt)
            ref = statement(inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'])
            s = stmt32(inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'])
            un, k = dict(ref['under']['exact']), k32[geom_class(c)]
            for name, v in (ref['wobble'] or {}).items():
                un[name] = un.get(name, 0.0) + v
            for name in ('grad', 'I', 'P', 'ce_sum', 'w_sum'):
                k[name] = max(k[name], worst(s[name], ref[name], name, ref['S_' + name], U24, un.get(name)))
            k['loss'] = max(k['loss'], worst(s['loss'], ref['loss'], 'loss', ref['S_loss'] + ref['S_loss_P'], U24))
            k['lse'] = max(k['lse'], worst(s['lse_full'], ref['lse_full'], 'lse', ref['lse_full'].abs().clamp_min(1.0), U24))
            if dt == BF and c['path'].startswith('r4'):
                b = stmt_bf16tile(inp['lo'], inp['t'], inp['cw'], c['go'], c['dice'])
                un = ref['under']['cell']
                kbf['grad'] = max(kbf['grad'], worst(b['grad'], ref['grad'], 'grad', ref['S_grad'], U9, un['grad']))
                kbf['P'] = max(kbf['P'], worst(b['P'], ref['P'], 'P', ref['S_P'], U9, un['P']))
    return k32, kbf


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
INPUT_CLASSES = ('plain', 'offset', 'offset_neg', 'confident', 'confident_wrong', 'const0', 'const', 'tiny', 'spike', 'spike_over', 'edge_class')
LABEL_KINDS = ('frame', 'stripes', 'stripes_off', 'image_ignored', 'absent', 'one_class', 'last', 'zero')
WEIGHT_KINDS = (None, 'ones', 'rand', 'spread', 'zero2')


def make_labels(kind, B, C, H, W, g):
    t = torch.randint(0, C, (B, H, W), generator=g)
    if kind == 'frame':
        t[:, :1] = IGNORE
        t[:, -1:] = IGNORE
        t[:, :, :1] = IGNORE
        t[:, :, -1:] = IGNORE
        if H <= 2 or W <= 2:                                        # the frame would leave nothing: keep one corner pixel per image
            t[:, 0, 0] = torch.arange(B) % C
    elif kind in ('stripes', 'stripes_off'):                        # cells start at Y % 4 == 2: aligned to the cell grid / off by one
        t[:, torch.arange(H) % 4 == (2 if kind == 'stripes' else 3)] = IGNORE
        t[:, :, torch.arange(W) % 4 == (2 if kind == 'stripes' else 3)] = IGNORE
        t[:, 0, 0] = 0
    elif kind == 'image_ignored':
        t[B - 1] = IGNORE
    elif kind == 'absent':
        if C > 1:
            t[0][t[0] == 1] = 0
    elif kind == 'one_class':
        t[:] = C // 2
    elif kind == 'last':
        t[:] = C - 1
    elif kind == 'zero':
        t[:] = 0
    elif kind == 'all_ignored':
        t[:] = IGNORE
    else:
        raise KeyError(kind)
    return t


def make_weights(kind, C, t, g):
    if kind is None:
        return None
    if kind == 'ones':
        return torch.ones(C)
    r = torch.rand(C, generator=g)
    if kind == 'rand':
        return r + 0.5
    if kind == 'spread':
        return torch.pow(10.0, 6 * r - 3)
    if kind == 'zero2':
        cw = r + 0.5
        present = torch.unique(t[t != IGNORE])
        cw[present[:2]] = 0.0
        return cw
    raise KeyError(kind)


def spike_tap(h, w):
    return min(h // 2, h - 1), min(w // 2, w - 1)


def make_logits(cls, B, C, h, w, t, g):
    """fp32 [B][C][h][w] of one input class (t: the labels, for the confident classes)."""
    H, W = t.shape[1:]
    z = torch.randn(B, C, h, w, generator=g)
    if cls == 'plain':
        return z * 2
    if cls in ('offset', 'offset_neg'):                              # steps of bf16 at 200: whole numbers, exact under dyadic tap weights
        return (z * 2 + (200 if cls == 'offset' else -200)).to(BF).float()
    if cls in ('confident', 'confident_wrong'):
        x = z * 0.1
        ys = ((torch.arange(h) + 0.5) * H / h).long().clamp_max(H - 1)
        xs = ((torch.arange(w) + 0.5) * W / w).long().clamp_max(W - 1)
        near = t[:, ys][:, :, xs]                                    # [B][h][w]: the label at the pixel nearest to the tap
        ok = near != IGNORE
        cl = torch.where(ok, near, torch.zeros_like(near))
        if cls == 'confident_wrong':
            cl = (cl + 1) % C
        x.scatter_add_(1, cl[:, None], 30.0 * ok[:, None].float())
        return x
    if cls == 'const0':
        return torch.zeros_like(z)
    if cls == 'const':
        return torch.full_like(z, -3.5)
    if cls == 'tiny':
        return z * 1e-4
    if cls in ('spike', 'spike_over'):                               # far on either side of the retry threshold, about 69 + ln C
        x = z * 0.5
        j, k = spike_tap(h, w)
        x[0, C // 3, j, k] = 50.0 if cls == 'spike' else 200.0
        return x
    if cls == 'edge_class':
        x = z * 0.1
        x[:, 0] += 12 + 3 * torch.randn(B, h, w, generator=g)
        x[:, C - 1] += 12 + 3 * torch.randn(B, h, w, generator=g)
        return x
    raise KeyError(cls)


def case(path, B, C, h, w, H, W, inp='plain', lab='frame', cwk=None, go=1.0, dice=True, ld='r8', env=None, note=''):
    """One row of a table.  ld: 'C' (unpadded rows), 'r8' (C rounded up to 8), 'r8+8', 'view8' (a column slice behind eight foreign
    columns), 'off4' (a slice whose first element is 8-byte but not 16-byte aligned in bf16)."""
    cid = f'{path}-B{B}C{C}-{h}x{w}to{H}x{W}-{inp}-{lab}-cw{cwk}-go{go:g}-{"dice" if dice else "ce"}-{ld}'
    return dict(id=cid, path=path, B=B, C=C, h=h, w=w, H=H, W=W, inp=inp, lab=lab, cw=cwk, go=go, dice=dice, ld=ld, env=dict(env or {}), note=note)


def inputs(c, dtype):
    """Labels, class weights and float64 logits (rounded to `dtype`) of one case; one seed per case id."""
    g = X.gen(seed_of(c['id']))
    t = make_labels(c['lab'], c['B'], c['C'], c['H'], c['W'], g)
    lo = make_logits(c['inp'], c['B'], c['C'], c['h'], c['w'], t, g)
    return dict(lo=to_storage(lo, dtype), t=t, cw=make_weights(c['cw'], c['C'], t, g))


# ---- paths: the switches that select them and the kernels they are meant to reach ------------------------------------------------
PATH_ENV = {
    'r1': {}, 'r2': {}, 'r8': {}, 'r4': {}, 'generic': {},
    'r4_nomfma': {'SEGFAC_LOSS_NO_MFMA': '1'},
    'r4_nolse': {'SEGFAC_LOSS_NO_LSE': '1'},
    'r4_rows8': {'SEGFAC_LOSS_BAND_ROWS': '8'},
    'r4_tile': {'SEGFAC_LOSS_NO_BAND_FWD': '1', 'SEGFAC_LOSS_NO_BAND': '1'},
}


def ld_of(c):
    r8 = (c['C'] + 7) // 8 * 8
    return {'C': (c['C'], 0), 'r8': (r8, 0), 'r8+8': (r8 + 8, 0), 'view8': (r8 + 8, 8), 'off4': (r8 + 8, 4)}[c['ld']]


def band_covers(c, dtype):
    """Does the band sweep take this case (loss_band_fwd_covers: bf16, ratio 4, rows a multiple of 8 elements, 16-byte aligned base)?"""
    ld, front = ld_of(c)
    return dtype == BF and c['path'] in ('r4', 'r4_nolse', 'r4_rows8') and ld % 8 == 0 and front % 8 == 0


def expected_kernels(c, dtype):
    """(forward, backward): the instantiated names (hip.trace) of the loss kernels the case must launch, in order; `loss_kernels`
    filters a trace down to them.  The per-pixel cell kernel behind a batched kernel is the exact-maximum retry pass."""
    T = ' [T = float]' if dtype == F32 else ' [T = unsigned short]'
    path, C = c['path'], c['C']
    NT, full = nt_bucket(C)
    ns = (C + 63) // 64
    fl = 'true' if full else 'false'
    retry_f, retry_b = f'ce_dice_fwd_cells_kernel<T, {ns}>{T}', f'ce_dice_bwd_cells_kernel<T, {ns}>{T}'
    if path == 'r1':
        return [retry_f], [retry_b]
    if path in ('r2', 'r8', 'r4_nomfma'):
        sc = {'r2': 2, 'r8': 8, 'r4_nomfma': 4}[path]
        return [f'ce_dice_fwd_cells16_kernel<T, {ns}, {sc}>{T}', retry_f], [f'ce_dice_bwd_cells8_kernel<T, {ns}, {sc}>{T}', retry_b]
    if path == 'generic':
        return [f'ce_dice_fwd_kernel<T, {ns}>{T}'], [f'ce_dice_bwd_kernel<T, {ns}>{T}', 'bilinear_bwd_kernel<T>']
    if band_covers(c, dtype):
        lse = 'false' if path == 'r4_nolse' else 'true'
        return [f'ce_dice_fwd_band_kernel<{NT}, {fl}>', retry_f], [f'ce_dice_bwd_band_kernel<{NT}, {fl}, {lse}>', retry_b]
    return [f'ce_dice_fwd_mfma4_kernel<T, {NT}>{T}', retry_f], [f'ce_dice_bwd_mfma4_kernel<T, {NT}>{T}', retry_b]


def loss_kernels(names):
    """A launch trace without the helpers (flag / pad zeroing, the partial-sum finalize, the loss scalar kernel)."""
    return [n for n in names if not n.startswith(('zero_ints_kernel', 'zero_words_kernel', 'colreduce_finalize_kernel', 'ce_dice_loss_kernel'))]


def has_retry(c):
    return c['path'] not in ('r1', 'generic')


# ---- tables --------------------------------------------------------------------------------------------------------------------------
R4_CLASS_COUNTS = (1, 2, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 160, 161, 191, 192)
R4_MAPS = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 7), (7, 8), (8, 8), (9, 9), (8, 15), (17, 14), (16, 22))
GENERIC_GEOMS = ((5, 6, 15, 18), (2, 3, 32, 48), (4, 6, 10, 27), (5, 7, 18, 23))          # ratios 3, 16, 2.5 x 4.5, (5, 7) -> (18, 23)


def _axes(path, B, C, h, w, H, W, full):
    """One axis at a time around the base case (path, B, C, h, w): inputs, labels, class weights, grad_out, dice, row strides."""
    out = [case(path, B, C, h, w, H, W)]
    pow2 = path != 'generic'
    for inp in (INPUT_CLASSES[1:] if full is not None else ('confident', 'spike_over')):
        if inp.startswith('offset') and not pow2:
            continue                  # not covered: outside the dyadic ratios the tap weights round 200 * 2^-24 into every logit
        if inp.startswith('spike') and h * w < 9:
            continue
        out.append(case(path, B, C, h, w, H, W, inp=inp, lab='one_class' if inp == 'edge_class' else 'frame'))
    if not full:                                            # False: every input class; None: the two hardest ones
        return out
    for lab in LABEL_KINDS[1:]:
        out.append(case(path, B, C, h, w, H, W, lab=lab))
    for cwk in WEIGHT_KINDS[1:]:
        out.append(case(path, B, C, h, w, H, W, cwk=cwk))
    for go in (1.7, 1024.0, 0.0):
        out.append(case(path, B, C, h, w, H, W, go=go, cwk='rand'))
    out.append(case(path, B, C, h, w, H, W, dice=False, cwk='rand', go=1.7))
    for ld in ('C', 'r8+8', 'view8', 'off4'):
        out.append(case(path, B, C, h, w, H, W, ld=ld))
    out.append(case(path, B, C, h, w, H, W, inp='confident', lab='image_ignored', cwk='spread', go=1.7))
    return out


def gpu_cases():
    """The rows the GPU tests run (each in fp32 and bf16 unless the path is one storage type's).  B <= 3, h, w <= 24, H, W <= 96."""
    out = []
    # ratio 4: every axis at C = 19 (default path and every switch), the inputs at C = 150
    for path in ('r4', 'r4_nomfma', 'r4_nolse', 'r4_tile'):
        out += _axes(path, 2, 19, 9, 10, 36, 40, full=path in ('r4', 'r4_tile'))
        out += _axes(path, 2, 150, 9, 10, 36, 40, full=None if path == 'r4_nomfma' else False)
    for C in R4_CLASS_COUNTS:
        for path in ('r4', 'r4_tile'):
            if C not in (19, 150):
                out.append(case(path, 2, C, 9, 10, 36, 40, cwk='rand', go=1.7))
    for C in (19, 150):
        for h, w in R4_MAPS:
            for path in ('r4', 'r4_tile'):
                out.append(case(path, 3 if h * w <= 81 else 2, C, h, w, 4 * h, 4 * w, cwk='rand', go=1.7, lab='stripes_off' if (h + w) % 2 else 'frame'))
    out.append(case('r4', 2, 150, 17, 14, 68, 56, inp='confident', cwk='rand'))
    out.append(case('r4_rows8', 2, 19, 17, 14, 68, 56, cwk='rand', go=1.7))
    out.append(case('r4_rows8', 2, 150, 17, 14, 68, 56, cwk='rand', go=1.7))
    # ratios 1, 2, 8
    for path, sc in (('r1', 1), ('r2', 2), ('r8', 8)):
        out += _axes(path, 2, 19, 5, 9, 5 * sc, 9 * sc, full=path == 'r2')
        for C in (19, 65, 150):
            for h, w in ((1, 1), (5, 9), (9, 8)):
                if (C, h, w) != (19, 5, 9):
                    out.append(case(path, 2, C, h, w, h * sc, w * sc, cwk='rand', go=1.7))
    # generic ratios
    for i, (h, w, H, W) in enumerate(GENERIC_GEOMS):
        out += _axes('generic', 2, 19, h, w, H, W, full=True if i == 0 else None)
        out.append(case('generic', 2, 150, h, w, H, W, cwk='rand', go=1.7))
        out.append(case('generic', 1, 65, h, w, H, W, lab='stripes'))
    seen = set()
    uniq = [c for c in out if not (c['id'] in seen or seen.add(c['id']))]
    for c in uniq:
        c['env'] = dict(PATH_ENV[c['path']])
    return uniq


def dtypes_of(c):
    """fp32 takes the band switches as no-ops: those rows run in bf16 only; the off4 stride is a bf16 alignment question."""
    if c['path'] in ('r4_nolse', 'r4_rows8', 'r4_tile'):
        return (BF,)
    return (F32, BF)


# small cases of the CPU tests (statement against autograd and the loop oracle, K, mutants): 2 x 19 x 8 x 8 -> 32 x 32 and variations
def cpu_cases():
    out = []
    for inp in INPUT_CLASSES:
        out.append(case('r4', 2, 19, 8, 8, 32, 32, inp=inp, lab='one_class' if inp == 'edge_class' else 'frame',
                        cwk='rand' if inp in ('plain', 'confident') else None))
    out += [case('r4', 2, 19, 8, 8, 32, 32, lab=lab, cwk='spread', go=1.7) for lab in LABEL_KINDS[1:]]
    out += [case('r4', 2, 19, 8, 8, 32, 32, cwk=k, go=1024.0) for k in WEIGHT_KINDS[1:]]
    out += [case('r4', 2, 19, 8, 8, 32, 32, dice=False, cwk='rand', go=1.7),
            case('r4', 3, 19, 5, 7, 20, 28, inp='confident', lab='image_ignored', cwk='spread', go=1.7),
            case('r4', 3, 19, 5, 7, 20, 28, inp='edge_class', lab='image_ignored', go=1.7),
            case('r4', 2, 19, 5, 7, 20, 28, inp='edge_class', lab='zero'),
            case('r2', 2, 5, 5, 9, 10, 18, cwk='rand'), case('r8', 1, 33, 3, 2, 24, 16, inp='confident'),
            case('r1', 2, 19, 5, 9, 5, 9, cwk='rand', go=1.7),
            case('generic', 2, 19, 5, 7, 18, 23, cwk='rand', go=1.7), case('generic', 2, 7, 4, 6, 10, 27, inp='confident')]
    return out
