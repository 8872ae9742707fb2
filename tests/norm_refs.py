"""Float64 statements of the norm and column-reduction operations (LayerNorm, BatchNorm on NHWC rows, GRN, colsum), their plain fp32
statements, the one comparator of tests/test_norm_float64.py and the input tables its GPU tests run.  Importable without a GPU.

Every reference takes its activations ALREADY ROUNDED to the storage type (`to_storage`), as float64; parameters are fp32 values.  The
formulas are those of include/segfac.h and of the comments of csrc/norm.hip, not a transcription of the kernels.

The comparator (`check`):  |got - ref64| <= half_ulp_T(ref64) + max(MARGIN * e_ref, FLOOR * 2^-24 * scale)   per element, where
  half_ulp_T  half a bf16 unit in the last place of ref64 for an output stored in bf16, 0 for one stored in fp32: the ONE rounding of the
              store;
  e_ref       the largest error, over the element's group, of the plain fp32 statement of the same operation on the same inputs against
              float64 (for a reduction: the larger of torch's `.sum(0)` and of the sequential fp32 sum, `seq_sum32`).  It is the
              reference's own error, never the kernel's;
  scale       elementwise outputs: the largest |ref64| of the group.  Reductions: the float64 sum of the absolute values of the terms.
              Statistics: stated at `ln_stat_scales` / `bn_stat_scales` (a mean IS a sum: the mean of the absolute values);
  MARGIN, FLOOR   per output class, `CLASSES`.
Where a case needs more, the larger factor or an additional term is DERIVED from the kernel's chain of additions, beside the case (every
use reads `DERIVED`; tests/test_norm_float64.py lists them).
A group is a row for LayerNorm outputs, a channel for BatchNorm outputs, an (image, channel) pair for GRN outputs, a column for reductions.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import exact_inputs as X

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24 = 2.0 ** -24                       # half a unit in the last place of an fp32 value in [1, 2)
# class -> (MARGIN, FLOOR)
#   elementwise outputs and per-row / per-channel statistics: the kernel and torch do the same two-pass fp32 arithmetic in another order;
#       the floor only matters where torch happens to be exact.
#   reductions: the sequential sum is already the worst-ordered standard algorithm.
CLASSES = {'elementwise': (4.0, 4.0), 'reduction': (2.0, 4.0)}
MAX_ELEMENTS = 9_000_000
GRN_EPS = 1e-6
KINK_ZONE = 64 * U24                   # ReLU / ReLU6: |pre - kink| <= KINK_ZONE * scale is left out of the dx comparison
DERIVED = True                         # False: the issue's bound alone, without the derived terms of single cases (for measurements)
KINK_CAP = 1e-3                        # at most 0.1 % of a tensor may be left out


def seed_of(name):
    return zlib.crc32(name.encode())


def to_storage(t, dtype):
    """fp32 / float64 values -> rounded to the storage type -> float64 (what the kernel reads)."""
    return t.to(F32).to(dtype).double()


def half_ulp(ref64, dtype):
    """Half a unit in the last place, in the storage type, of each float64 value: 0 for fp32 storage (the fp32 statement pays that rounding
    as well), 2^(e - 9) for a bf16 value m 2^e with m in [0.5, 1)."""
    if dtype != BF:
        return torch.zeros_like(ref64)
    _, e = torch.frexp(ref64.abs().clamp_min(2.0 ** -126))
    return torch.where(ref64 == 0, torch.zeros_like(ref64), torch.ldexp(torch.ones_like(ref64), e - 9))


def _grp(v, like):
    """Per-group value (a number, or a tensor that broadcasts against `like`: keepdim shapes) expanded to `like`."""
    return torch.as_tensor(v, dtype=F64).expand_as(like)


class Verdict:
    """Outcome of one comparison: ok, the largest observed (err - half_ulp) / max(e_ref, FLOOR / MARGIN * 2^-24 * scale) -- the number that
    must stay at or below MARGIN -- and the message of a failure."""

    def __init__(self, ok, ratio, message):
        self.ok, self.ratio, self.message = ok, ratio, message

    def __bool__(self):
        return self.ok


def compare(got, ref64, e_ref, scale, storage_dtype, cls='elementwise', what='', margin=None, floor=None, extra=None, keep=None):
    """The comparator, as a Verdict.  e_ref, scale (and floor / extra where given) are per group: a number, a tensor of the leading
    dimensions of ref64 (rows of a [rows][C] output), or anything that broadcasts against ref64 (shape [1][C]: per column).
    margin / floor: the class values unless a case DERIVES larger ones (written beside the case).  extra: a derived absolute term added
    to the max (a conditioning term that e_ref cannot carry because the fp32 statement does not share it).  keep: bool mask of the
    elements that are compared (ReLU kinks)."""
    m, f = CLASSES[cls]
    margin = m if margin is None else margin
    floor = f if floor is None else floor
    ref64 = ref64.detach().double().cpu()
    g = got.detach().double().cpu().reshape(ref64.shape)
    e_ref, scale, floor = _grp(e_ref, ref64), _grp(scale, ref64), _grp(floor, ref64)
    slack = torch.maximum(margin * e_ref, floor * U24 * scale)
    if extra is not None:
        slack = slack + _grp(extra, ref64)
    hu = half_ulp(ref64, storage_dtype)
    err = (g - ref64).abs()
    bad = ~(err <= hu + slack)                               # a NaN or an infinity is never inside the bound
    if keep is not None:
        bad &= keep
    unit = slack / margin
    ratio = torch.where(unit > 0, (err - hu).clamp_min(0) / unit, torch.where(err > hu, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(err, math.inf))
    if keep is not None:
        ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not bad.any():
        return Verdict(True, worst, '')
    i = int(torch.where(bad.reshape(-1), ratio.reshape(-1), torch.full_like(ratio.reshape(-1), -1.0)).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref64.shape)) if ref64.dim() else ()
    f1 = lambda t: t.reshape(-1)[i].item()                   # noqa: E731
    er = f1(e_ref)
    want = torch.where(bad, ref64, g).to(got.dtype if got.dtype in (BF, F32) else F32)
    msg = (f'{what}: group / element {idx}: got {f1(g)!r}, float64 {f1(ref64)!r}, |err| {f1(err):.4g} > half ulp {f1(hu):.4g} + '
           f'max({margin:g} * e_ref {er:.4g}, {f1(floor):g} * 2^-24 * scale {f1(scale):.4g})'
           f'{"" if extra is None else f" + derived {f1(_grp(extra, ref64)):.4g}"}; err / e_ref = '
           f'{(f1(err) / er if er > 0 else math.inf):.4g}, allowed {margin:g}\n'
           + (X.mismatch_report(g.to(want.dtype), want, what) or ''))
    return Verdict(False, worst, msg)


def check(got, ref64, e_ref, scale, storage_dtype, cls='elementwise', what='', **kw):
    v = compare(got, ref64, e_ref, scale, storage_dtype, cls, what, **kw)
    assert v.ok, v.message
    return v.ratio


def group_err(stmt32, ref64, dim):
    """e_ref of an elementwise output: the largest |fp32 statement - float64| over `dim` (kept, so that it broadcasts)."""
    e = (stmt32.detach().double() - ref64).abs()
    return e.amax(dim, keepdim=True) if dim is not None else e


def group_max(ref64, dim):
    return ref64.abs().amax(dim, keepdim=True)


# ---- column sums ------------------------------------------------------------------------------------------------------------------
def colsum_ref(x64):
    return x64.sum(0)


def seq_sum32(t32):
    """The plain sequential fp32 column sum: row after row into one fp32 accumulator per column.  (torch's CPU `cumsum` is NOT that: it
    keeps its running sum of fp32 data in double, so `cumsum(0)[-1]` is the correctly rounded sum; numpy's accumulates in the array's type.
    test_sequential_sum_is_sequential_fp32 pins this.)"""
    a = t32.detach().to(F32).contiguous().numpy()
    return torch.from_numpy(np.cumsum(a, axis=0, dtype=np.float32)[-1].copy())


def fp32_sums(t32):
    """The two fp32 statements of a column sum: torch's `.sum(0)` and the plain sequential sum."""
    t32 = t32.detach().to(F32)
    return t32.sum(0), seq_sum32(t32)


def sums_err(terms32, ref64):
    """e_ref of a column sum: the larger error of the two fp32 sums of the fp32 terms."""
    a, b = fp32_sums(terms32)
    return torch.maximum((a.double() - ref64).abs(), (b.double() - ref64).abs())


def cr_roundings(rows, C):
    """Roundings on the longest way of a term through the two-stage column reduction of csrc/colreduce.h, restating cr_plan: a thread adds
    its rows two at a time (v + w, then the accumulator), the rl row lanes of a block are added one after the other, the finalize adds every
    16th block partial and then its 16 slices.  |error of the sum| <= cr_roundings * 2^-24 * sum |terms| (first order)."""
    nchunk = -(-C // 8)
    ch = min(nchunk, 256)
    if 256 % ch:
        ch = next((c2 for c2 in (64, 32, 16, 8) if nchunk % c2 == 0), ch)
    rl, slabs = 256 // ch, -(-nchunk // ch)
    nblk = max(1, min(-(-rows // (rl * 32)), max(2048 // slabs, 1)))
    per_thread = -(-(-(-rows // nblk)) // rl)
    return (-(-per_thread // 2) + 1) + rl + -(-nblk // 16) + 16


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, gamma, beta, eps):
    """y = (x - mean) * rstd * gamma + beta over the last dim; rstd = 1 / sqrt(biased variance + eps).  -> (y, mean [rows], rstd [rows])."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    return (x - mean) * rstd * gamma.double() + beta.double(), mean[:, 0], rstd[:, 0]


def ln_bwd_ref(x, dy, gamma, eps, dy2=None, dres=None, rscale=None, rows_per_group=1, dtype=F32):
    """dx = LN_bwd(dy + dy2) + dres, dgamma = sum_rows g * xhat, dbeta = sum_rows g (g = dy + dy2), and, with rscale,
    dxs = round_T(dx) * rscale[row // rows_per_group].  -> dict(dx, dgamma, dbeta, dxs, terms_g, terms_b)."""
    _, mean, rstd = ln_fwd_ref(x, gamma, beta=torch.zeros_like(gamma), eps=eps)
    g = dy if dy2 is None else dy + dy2
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = g * gamma.double()
    dx = rstd[:, None] * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres
    out = dict(dx=dx, dgamma=(g * xh).sum(0), dbeta=g.sum(0), terms_g=g * xh, terms_b=g, dxs=None)
    if rscale is not None:
        out['dxs'] = scaled_from_stored(to_storage(dx, dtype), rscale, rows_per_group)
    return out


def scaled_from_stored(dx_stored64, rscale, rows_per_group):
    """dxs of the STORED dx (already rounded to the storage type): dx * rscale[row // rows_per_group]."""
    r = torch.arange(dx_stored64.shape[0]) // rows_per_group
    return dx_stored64 * rscale.double()[r][:, None]


def ln_fp32(x32, gamma, beta, eps, dy32=None, dy2_32=None, dres32=None):
    """The fp32 statement: F.layer_norm on fp32 CPU tensors, with autograd.  mean / rstd (which F.layer_norm does not return): torch's
    fp32 `mean` and `var(unbiased=False)`.  -> dict(y, mean, rstd[, dx, dgamma, dbeta])."""
    xr = x32.clone().requires_grad_(dy32 is not None)
    gr, br = gamma.clone().requires_grad_(dy32 is not None), beta.clone().requires_grad_(dy32 is not None)
    y = F.layer_norm(xr, (x32.shape[1],), gr, br, eps)
    mean = x32.mean(-1)
    out = dict(y=y.detach(), mean=mean, rstd=torch.rsqrt(x32.var(-1, unbiased=False) + eps))
    if dy32 is not None:
        g = dy32 if dy2_32 is None else dy32 + dy2_32
        y.backward(g)
        out.update(dx=xr.grad if dres32 is None else xr.grad + dres32, dgamma=gr.grad, dbeta=br.grad, g=g,
                   xhat=(x32 - mean[:, None]) * out['rstd'][:, None])
    return out


def ln_stat_scales(x, rstd64):
    """Scales of the per-row statistics.  mean: it is the sum of the terms x / C, so its scale is that of a reduction, sum |x| / C (|mean|
    itself can be arbitrarily small against the terms that are added).  rstd: |rstd| (a sum of squares cancels nothing)."""
    return x.abs().mean(-1), rstd64.abs()


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------
def bn_stats_ref(x, eps, rmean0, rvar0, momentum):
    """Training statistics in float64 (two-pass: the variance is that of the centred data)."""
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    unb = var * n / (n - 1) if n > 1 else var
    return (mean, 1.0 / torch.sqrt(var + float(eps)), (1 - momentum) * rmean0.double() + momentum * mean,
            (1 - momentum) * rvar0.double() + momentum * unb)


def bn_stats_fp32(x32, eps, rmean0, rvar0, momentum):
    """The documented algorithm, twice: fp32 column sums of x and x * x (torch's `.sum(0)`, then the sequential sum), combined in float64;
    the results are stored as fp32 and the running statistics are updated in fp32.  -> [(mean, rstd, rmean, rvar)] * 2."""
    return [bn_from_sums32(s1, s2, x32.shape[0], eps, rmean0, rvar0, momentum) for s1, s2 in zip(fp32_sums(x32), fp32_sums(x32 * x32))]


def bn_from_sums32(s1, s2, n, eps, rmean0, rvar0, momentum, mut=None):
    """fp32 sums -> float64 combine -> fp32 (mean, rstd, running_mean, running_var).  mut: a wrong computation (MUTANTS)."""
    mean = s1.double() / n
    var = (s2.double() / n - mean * mean).clamp_min(0)
    unb = var * n / (n - 1) if n > 1 else var
    vr = unb if mut == 'rstd_unbiased' else var
    rstd = 1.0 / (torch.sqrt(vr) + eps) if mut == 'eps_outside' else 1.0 / torch.sqrt(vr) if mut == 'eps_dropped' else 1.0 / torch.sqrt(vr + eps)
    m32, r32 = mean.float(), rstd.float()
    if mut == 'mean_bf16':
        m32 = m32.to(BF).float()
    if mut == 'rstd_bf16':
        r32 = r32.to(BF).float()
    return (m32, r32, (1 - momentum) * rmean0 + momentum * m32,
            (1 - momentum) * rvar0 + momentum * (var if mut == 'running_biased' else unb).float())


def bn_stat_scales(x, ref):
    """Scales of (mean, rstd, running_mean, running_var): the mean is a sum of x / n (scale: the mean of |x|); the others their own size."""
    mean, rstd, rm, rv = ref
    return x.abs().mean(0), rstd.abs(), rm.abs(), rv.abs()      # (bn_yard replaces the third: it needs the starting value)


def _act(v, act):
    return v.clamp(min=0) if act == 1 else v.clamp(min=0, max=6) if act == 2 else v


def _act_mask(pre, act):
    if act == 1:
        return (pre > 0).to(pre.dtype)
    if act == 2:
        return ((pre > 0) & (pre < 6)).to(pre.dtype)
    return torch.ones_like(pre)


def _cs_rows(chan_scale, rows, rps, dtype):
    if chan_scale is None:
        return None
    return chan_scale.to(dtype)[torch.arange(rows) // rps]


def bn_apply_ref(x, mean, rstd, gamma, beta, act, chan_scale=None, rps=1):
    """y = act(gamma * (x - mean) * rstd + beta) * chan_scale[row // rows_per_sample][c] for GIVEN mean / rstd.  -> (y, pre-activation)."""
    t = x.dtype
    pre = (x - mean.to(t)) * rstd.to(t) * gamma.to(t) + beta.to(t)
    y = _act(pre, act)
    cs = _cs_rows(chan_scale, x.shape[0], rps, t)
    return (y if cs is None else y * cs), pre


def bn_bwd_ref(x, dy, mean, rstd, gamma, beta, act, chan_scale=None, rps=1, eval_mode=False):
    """d = dy * chan_scale * act'(pre); dbeta = sum d; dgamma = sum d * xhat; dx = gamma * rstd * (d - [training] (dbeta + xhat * dgamma) / n)
    for GIVEN mean / rstd.  -> dict(dx, dgamma, dbeta, terms_g, terms_b, pre)."""
    t = x.dtype
    xh = (x - mean.to(t)) * rstd.to(t)
    pre = xh * gamma.to(t) + beta.to(t)
    d = dy * _act_mask(pre, act)
    cs = _cs_rows(chan_scale, x.shape[0], rps, t)
    if cs is not None:
        d = d * cs
    db, dg = d.sum(0), (d * xh).sum(0)
    inner = d if eval_mode else d - db / x.shape[0] - xh * (dg / x.shape[0])
    return dict(dx=gamma.to(t) * rstd.to(t) * inner, dgamma=dg, dbeta=db, terms_g=d * xh, terms_b=d, pre=pre)


def kink_zone(pre64, act):
    """Elements whose float64 pre-activation lies within KINK_ZONE * (largest |pre| of the channel) of a kink (0; 6 for ReLU6) without
    lying ON it: there the fp32 sign of `pre` is not determined.  An element exactly on a kink is not in the zone: the inputs that put
    it there (the `lattice` class) make the fp32 value exact too, and the derivative on the kink is 0 by definition."""
    if act == 0:
        return torch.zeros_like(pre64, dtype=torch.bool)
    tol = KINK_ZONE * pre64.abs().amax(0, keepdim=True)
    z = (pre64.abs() <= tol) & (pre64 != 0)
    if act == 2:
        z |= ((pre64 - 6).abs() <= tol) & (pre64 != 6)
    return z


# ---- GRN --------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def grn_fwd_ref(x, gamma, beta, B, pre_gelu=False):
    """x [B * P][C]; a = gelu(x) when pre_gelu.  Gx[b][c] = sqrt(sum_p a^2), Nx = Gx / (mean_c Gx + 1e-6), y = gamma * (a * Nx) + beta + a.
    -> (y, sums [B][C] of a^2, the terms a^2 [B][P][C])."""
    C = x.shape[1]
    a = (gelu64(x) if pre_gelu else x).reshape(B, -1, C)
    sq = (a * a).sum(1)
    G = torch.sqrt(sq)
    Nx = G / (G.mean(-1, keepdim=True) + GRN_EPS)
    y = gamma.double() * (a * Nx[:, None]) + beta.double() + a
    return y.reshape(-1, C), sq, a * a


def grn_bwd_ref(x, dy, gamma, B, pre_gelu=False):
    """With A = gamma * sum_p dy * a, m = mean_c Gx + 1e-6:  dL/dGx = A / m - (1 / C) sum_c' A Gx / m^2,  K = Gx > 0 ? dL/dGx / Gx : 0
    (sqrt(0) has gradient 0),  da = (1 + gamma Nx) dy + K a,  dx = da * gelu'(x) when pre_gelu;  dgamma = sum_b Nx sum_p dy a,
    dbeta = sum dy.  -> dict(dx, dgamma, dbeta, terms_g [B][C], terms_b [B * P][C])."""
    C = x.shape[1]
    a = (gelu64(x) if pre_gelu else x).reshape(B, -1, C)
    d = dy.reshape(B, -1, C)
    G = torch.sqrt((a * a).sum(1))
    m = G.mean(-1, keepdim=True) + GRN_EPS
    Nx = G / m
    S1 = (d * a).sum(1)
    A = gamma.double() * S1
    dG = A / m - (A * G).sum(-1, keepdim=True) / (C * m * m)
    K = torch.where(G > 0, dG / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    da = (1 + gamma.double() * Nx)[:, None] * d + K[:, None] * a
    dx = da.reshape(-1, C)
    if pre_gelu:
        dx = dx * gelu_grad64(x)
    return dict(dx=dx, dgamma=(Nx * S1).sum(0), dbeta=dy.sum(0), terms_g=Nx * S1, terms_b=dy)


def grn_module(x4, gamma, beta):
    """The GRN module of ConvNeXtV2, literally (x4: [B][H][W][C], any float type, autograd)."""
    Gx = torch.norm(x4, p=2, dim=(1, 2), keepdim=True)
    Nx = Gx / (Gx.mean(dim=-1, keepdim=True) + GRN_EPS)
    return gamma * (x4 * Nx) + beta + x4


def grn_fp32(x32, gamma, beta, B, pre_gelu=False, dy32=None):
    """The fp32 statement: F.gelu and the literal module on fp32 CPU tensors, with autograd.  -> dict(y, sq[, dx, dgamma, dbeta])."""
    C = x32.shape[1]
    xr = x32.clone().requires_grad_(dy32 is not None)
    gr, br = gamma.clone().requires_grad_(dy32 is not None), beta.clone().requires_grad_(dy32 is not None)
    a = (F.gelu(xr) if pre_gelu else xr).reshape(B, -1, 1, C)
    y = grn_module(a, gr, br).reshape(-1, C)
    ad = a.detach().reshape(B, -1, C)
    out = dict(y=y.detach(), a=ad)
    if dy32 is not None:
        y.backward(dy32)
        out.update(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    return out


# ---- the input tables of the GPU tests --------------------------------------------------------------------------------------------
def _randn(shape, g):
    return torch.randn(tuple(shape), generator=g, dtype=F32)


def _dyadic(n, g):
    """n constants k / 4, |k| <= 24, no two neighbours equal: exact in bf16, and every partial sum of up to 2^17 of them is exact in fp32, so
    the fp32 mean of a constant group IS the constant in any summation order and eps alone decides the result."""
    k = torch.randint(-24, 25, (n,), generator=g)
    k = torch.where(k == torch.roll(k, 1), k + 1, k)
    return k.float() / 4


def make_x(cls, rows, C, g, group_dim):
    """Activations of one input class.  group_dim: 1 = a group is a row (LayerNorm), 0 = a group is a column (BatchNorm, colsum)."""
    z = _randn((rows, C), g)
    ngroups = rows if group_dim == 1 else C
    if cls == 'plain':
        return z * 2 + 0.5
    if cls == 'offset':
        return z + 100
    if cls == 'offset8':
        return z + 8
    if cls == 'offset30':
        return z + 30
    if cls == 'big':
        return z * 1e4
    if cls == 'tiny':
        return z * 1e-3
    if cls == 'const':
        c = _dyadic(ngroups, g)
        return (c[:, None] if group_dim == 1 else c[None, :]).expand(rows, C).clone()
    if cls == 'outlier':
        x = z * 0.01
        pos = torch.randint(0, C if group_dim == 1 else rows, (ngroups,), generator=g)
        if group_dim == 1:
            x[torch.arange(rows), pos] = 50.0
        else:
            x[pos, torch.arange(C)] = 50.0
        return x
    raise KeyError(cls)


LN_CLASSES = ('plain', 'offset', 'big', 'tiny', 'const', 'outlier')
# (rows, C) of the `plain`-only cases and what each reaches in csrc/norm.hip
LN_PLAIN_SHAPES = (
    (67, 8, 'one lane per row, ragged last wave'),
    (37, 24, 'an idle fourth lane'),
    (9, 520, 'second chunk step with 63 idle lanes'),
    (5, 3072, 'six steps; the 96 KB LDS backward'),
    (1, 64, 'one row'),
    (4101, 512, 'b4 = 257: four row groups per wave, ragged last pass'),
    (16391, 512, 'forward grid-stride second pass at 4096 blocks; backward at the 1024-block cap'),
)


def ln_cases():
    """[dict(id, rows, C, cls, eps, fan)]: all classes at (333, 40) and (67, 520) with eps 1e-5 and 1e-6; `plain` at LN_PLAIN_SHAPES
    (eps 1e-5; 1e-6, ConvNeXt's, at the two widths that only ConvNeXt has); the fan-in form at (333, 40)."""
    out = []
    for rows, C in ((333, 40), (67, 520)):
        for cls in LN_CLASSES:
            for eps in (1e-5, 1e-6):
                out.append(dict(id=f'ln-{cls}-{rows}x{C}-eps{eps:g}', rows=rows, C=C, cls=cls, eps=eps, fan=False))
    for rows, C, _ in LN_PLAIN_SHAPES:
        eps = 1e-6 if C in (520, 3072) else 1e-5
        out.append(dict(id=f'ln-plain-{rows}x{C}-eps{eps:g}', rows=rows, C=C, cls='plain', eps=eps, fan=False))
    out.append(dict(id='ln-fanin-333x40-eps1e-05', rows=333, C=40, cls='plain', eps=1e-5, fan=True))
    return out


LN_RPG = 37           # rows_per_group of the fan-in case's rscale


def ln_inputs(case, dtype):
    """float64 inputs (activations rounded to `dtype`) and fp32 parameters of one LayerNorm case."""
    g = X.gen(seed_of(case['id']))
    rows, C = case['rows'], case['C']
    d = dict(x=to_storage(make_x(case['cls'], rows, C, g, 1), dtype), gamma=1 + 0.5 * _randn((C,), g), beta=0.5 * _randn((C,), g),
             dy=to_storage(_randn((rows, C), g), dtype), dy2=None, dres=None, rscale=None)
    if case['fan']:
        d.update(dy2=to_storage(_randn((rows, C), g), dtype), dres=to_storage(_randn((rows, C), g), dtype),
                 rscale=torch.rand(-(-rows // LN_RPG), generator=g) + 0.5)
    return d


BN_SHAPES = ((1, 72), (2, 72), (150, 19), (4101, 72), (4101, 768), (1367, 2304))
BN_CLASSES = ('plain', 'tiny', 'const', 'outlier', 'offset8', 'offset30')
BN_MOMENTUM = 0.1
BN_EPS = 1e-5


def bn_cases():
    """[dict(id, rows, C, cls, act, rps)]: every class at every shape with ReLU; act 0 and ReLU6 as well at (4101, 72); chan_scale [3][C]
    with rows_per_sample = rows / 3 where 3 divides rows.  Plus `lattice` (see bn_inputs) for the masks ON the kinks."""
    out = []
    for rows, C in BN_SHAPES:
        for cls in BN_CLASSES:
            for act in ((0, 1, 2) if (rows, C) == (4101, 72) else (1,)):
                out.append(dict(id=f'bn-{cls}-{rows}x{C}-act{act}', rows=rows, C=C, cls=cls, act=act, rps=rows // 3 if rows % 3 == 0 else 0))
    for act in (1, 2):
        out.append(dict(id=f'bn-lattice-150x24-act{act}', rows=150, C=24, cls='lattice', act=act, rps=50))
    return out


def bn_inputs(case, dtype):
    """float64 inputs and fp32 parameters of one BatchNorm case.  One channel has gamma = 0; 0.25 <= |beta| <= 0.75.  ReLU6 cases have a three times larger gamma, so
    that the upper kink is reached.  Class `lattice`: x integers in [-8, 8], gamma in {1, 2, 0.5}, beta integers, to be used with the GIVEN
    statistics mean = 0, rstd = 1: every pre-activation is an exact small multiple of 1 / 2 in every precision and many lie ON 0 and 6."""
    g = X.gen(seed_of(case['id']))
    rows, C, act = case['rows'], case['C'], case['act']
    if case['cls'] == 'lattice':
        x = torch.randint(-8, 9, (rows, C), generator=g).float()
        gamma = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (C,), generator=g)]
        beta = torch.randint(-2, 3, (C,), generator=g).float()
    else:
        x = make_x(case['cls'], rows, C, g, 0)
        gamma = (1 + 0.5 * _randn((C,), g)) * (3.0 if act == 2 else 1.0)
        # |beta| >= 0.25: where a group's spread is small against its largest element (`outlier`, `tiny`, `const`) whole channels would
        # otherwise sit inside the kink zone, which is sized by the largest pre-activation (the cap of test_kink_cap)
        beta = (0.25 + 0.5 * torch.rand(C, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (C,), generator=g).float())
    gamma[C // 2] = 0.0
    return dict(x=to_storage(x, dtype), gamma=gamma, beta=beta, dy=to_storage(_randn((rows, C), g), dtype),
                chan_scale=(torch.rand(3, C, generator=g) * 1.5 + 0.25) if case['rps'] else None,
                rmean0=0.3 * _randn((C,), g), rvar0=torch.rand(C, generator=g) + 0.5)


GRN_B = 3
GRN_SHAPES = ((1, 8), (49, 40), (1367, 768))
GRN_CLASSES = ('plain', 'big', 'tiny', 'zero_channel', 'zero_image')


def grn_cases():
    return [dict(id=f'grn-{cls}-{rps}x{C}-{"gelu" if pg else "id"}', rps=rps, C=C, cls=cls, pre_gelu=pg)
            for rps, C in GRN_SHAPES for cls in GRN_CLASSES for pg in (False, True)]


def grn_inputs(case, dtype):
    """plain: randn * 2 + 0.5; big: * 1e3; tiny: * 1e-4 (the 1e-6 beside the mean of Gx decides); zero_channel: one channel all zero in
    every image; zero_image: one whole image all zero."""
    g = X.gen(seed_of(case['id']))
    rps, C, cls = case['rps'], case['C'], case['cls']
    x = (_randn((GRN_B * rps, C), g) * 2 + 0.5) * {'big': 1e3, 'tiny': 1e-4}.get(cls, 1.0)
    if cls == 'zero_channel':
        x[:, C // 3] = 0
    if cls == 'zero_image':
        x[rps:2 * rps] = 0
    return dict(x=to_storage(x, dtype), gamma=0.5 * _randn((C,), g), beta=0.1 * _randn((C,), g),
                dy=to_storage(_randn((GRN_B * rps, C), g), dtype))


COLSUM_SHAPES = ((1, 72), (2, 19), (4101, 72), (4101, 768), (70001, 40), (300, 3080))
COLSUM_CLASSES = ('plain', 'positive', 'offset', 'alternating')


def colsum_cases():
    return [dict(id=f'colsum-{cls}-{rows}x{cols}', rows=rows, cols=cols, cls=cls) for rows, cols in COLSUM_SHAPES for cls in COLSUM_CLASSES]


def colsum_inputs(case, dtype):
    """plain; positive: randn ** 2; offset: randn + 1000; alternating: rows of +1e4 / -1e4 in turn, plus randn * 0.01."""
    g = X.gen(seed_of(case['id']))
    rows, cols, cls = case['rows'], case['cols'], case['cls']
    z = _randn((rows, cols), g)
    if cls == 'plain':
        x = z * 2 + 0.5
    elif cls == 'positive':
        x = z ** 2
    elif cls == 'offset':
        x = z + 1000
    else:
        sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
        x = sign[:, None] * 1e4 + z * 0.01
    return dict(x=to_storage(x, dtype))


def case_elements(case):
    if 'cols' in case:
        return case['rows'] * case['cols']
    if 'rps' in case and 'rows' not in case:
        return GRN_B * case['rps'] * case['C']
    return case['rows'] * case['C']


# ---- fp32 statements written out step by step (torch ops on fp32 CPU tensors), with the wrong computations of MUTANTS ---------------------
def _drop_or_twice(terms, mut):
    """Column sum of fp32 terms [rows][...] with the last row dropped / counted twice."""
    s = terms.sum(0)
    return s - terms[-1] if mut == 'last_row_dropped' else s + terms[-1] if mut == 'last_row_twice' else s


def _store(t32, dtype):
    return t32.to(dtype)


def ln_manual32(inp, case, dtype, mut=None):
    """LayerNorm forward and backward in plain two-pass fp32.  -> the outputs of the kernels' wrappers (y, dx, dxs in the storage type)."""
    x, dy = inp['x'].float(), inp['dy'].float()
    gamma, beta, eps = inp['gamma'], inp['beta'], case['eps']
    C = x.shape[1]
    if mut == 'chunk_prev_row':                     # the last 8-channel chunk of every row is read from the row before
        x = x.clone()
        x[1:, C - 8:] = inp['x'].float()[:-1, C - 8:]
    width = C
    if mut == 'mean_padded_width':                  # C rounded up to the lanes that share a row: 8 elements x the next power of two
        lanes = 1
        while lanes < C // 8 and lanes < 64:
            lanes *= 2
        width = -(-(C // 8) // lanes) * lanes * 8
    mean = x.sum(-1, keepdim=True) / width
    if mut == 'mean_bf16':
        mean = mean.to(BF).float()
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / C
    rstd = 1 / (var.sqrt() + eps) if mut == 'eps_outside' else var.rsqrt() if mut == 'eps_dropped' else (var + eps).rsqrt()
    if mut == 'rstd_bf16':
        rstd = rstd.to(BF).float()
    xh = (x - mean) * rstd
    out = dict(y=_store(xh * gamma + beta, dtype), mean=mean[:, 0], rstd=rstd[:, 0])
    g = dy if inp['dy2'] is None or mut == 'dy2_ignored' else dy + inp['dy2'].float()
    gy = g * gamma
    inner = gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True)
    dres = None if inp['dres'] is None else inp['dres'].float()
    dx = rstd * inner if dres is None else rstd * (inner + dres) if mut == 'dres_before_rstd' else rstd * inner + dres
    out.update(dx=_store(dx, dtype), dgamma=_drop_or_twice(g * ((x - mean) if mut == 'dgamma_no_rstd' else xh), mut),
               dbeta=_drop_or_twice(g, mut), dxs=None)
    if inp['rscale'] is not None:
        sc = inp['rscale'][torch.arange(x.shape[0]) // LN_RPG][:, None]
        out['dxs'] = _store(dx * sc, dtype) if mut == 'dxs_unrounded' else _store(out['dx'].float() * sc, dtype)
    return out


def bn_manual32(inp, case, dtype, mut=None, given=None):
    """bn_stats -> bn_apply -> bn_bwd (training and eval) in fp32, the later steps on the statistics of the first (or on `given`)."""
    x, dy, gamma, beta = inp['x'].float(), inp['dy'].float(), inp['gamma'], inp['beta']
    n, act, rps, cs = x.shape[0], case['act'], case['rps'], inp['chan_scale']
    s1, s2 = _drop_or_twice(x, mut), _drop_or_twice(x * x, mut)
    mean, rstd, rm, rv = bn_from_sums32(s1, s2, n, BN_EPS, inp['rmean0'], inp['rvar0'], BN_MOMENTUM, mut)
    if given is not None:
        mean, rstd = given
    out = dict(mean=mean, rstd=rstd, rmean=rm, rvar=rv)
    rps_used = rps + 1 if (mut == 'rps_off_by_one' and rps) else rps
    out['y'] = _store(bn_apply_ref(x, mean, rstd, gamma, beta, act, cs, max(rps_used, 1))[0], dtype)
    for mode in (False, True):
        xh = (x - mean) * rstd
        pre = xh * gamma + beta
        mask = ((pre > 0) & (pre <= 6)).float() if (mut == 'relu6_closed_at_6' and act == 2) else _act_mask(pre, act)
        d = dy * mask
        if cs is not None:
            d = d * _cs_rows(cs, n, max(rps, 1), F32)
        db, dg = d.sum(0), (d * xh).sum(0)
        inner = d if mode else d - db / n - xh * (dg / n)
        out['eval' if mode else 'train'] = dict(dx=_store(gamma * rstd * inner, dtype), dgamma=dg, dbeta=db)
    return out


def gelu32(x):
    return 0.5 * x * (1 + torch.erf(x * (1 / math.sqrt(2.0))))


def grn_manual32(inp, case, dtype, mut=None):
    x, dy, gamma, beta = inp['x'].float(), inp['dy'].float(), inp['gamma'], inp['beta']
    C, B = x.shape[1], GRN_B
    a = (gelu32(x) if case['pre_gelu'] else x).reshape(B, -1, C)
    d = dy.reshape(B, -1, C)
    sq = (a * a).sum(1)
    G = sq.sqrt()
    m = G.sum(-1, keepdim=True) / ((C - 1) if mut == 'mean_over_c_minus_1' else C)
    inv = 1 / m if mut == 'eps_dropped' else 1 / (m + GRN_EPS)
    Nx = G * inv
    y = a * (1 + gamma * Nx)[:, None] + beta
    S1 = (d * a).sum(1)
    A = gamma * S1
    dG = A * inv - (A * G).sum(-1, keepdim=True) * inv * inv / C
    K = dG / G if mut == 'k_not_zeroed' else torch.where(G > 0, dG / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    dx = ((1 + gamma * Nx)[:, None] * d + K[:, None] * a).reshape(-1, C)
    if case['pre_gelu']:
        dx = dx * (0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi))
    return dict(y=_store(y.reshape(-1, C), dtype), sq=sq, dx=_store(dx, dtype), dgamma=(Nx * S1).sum(0), dbeta=d.sum((0, 1)),
                terms_g=(Nx[:, None] * d * a).reshape(-1, C), terms_sq=a * a)


def colsum_manual32(inp, case, dtype, mut=None):
    x = inp['x'].float()
    if mut == 'partial_bf16':                       # four row blocks; the first block's partial sum passes through bf16
        parts = [p.sum(0) for p in torch.chunk(x, 4, 0)]
        return dict(sum=sum(parts[1:], parts[0].to(BF).float()))
    return dict(sum=_drop_or_twice(x, mut))


# ---- yardsticks (float64 result, e_ref, scale of every output of a case) and judges --------------------------------------------------
class Yard(dict):
    __getattr__ = dict.__getitem__


def _entry(ref, e, scale, store, cls='elementwise', keep=None):
    return dict(ref=ref, e=e, scale=scale, store=store, cls=cls, keep=keep)


def judge(entries, got, what, only=None):
    """{output: Verdict} of the outputs of `got` that have an entry (and are named by `only`)."""
    out = {}
    for name, en in entries.items():
        if (only is None or name in only) and got.get(name) is not None:
            out[name] = compare(got[name], en['ref'], en['e'], en['scale'], en['store'], en['cls'], f'{what} {name}', keep=en['keep'],
                                margin=en.get('margin'), floor=en.get('floor'), extra=en.get('extra'))
    return out


def _sum_entry(terms64, terms32, more32=()):
    ref = terms64.sum(0)
    e = sums_err(terms32, ref)
    for m in more32:
        e = torch.maximum(e, (m.detach().double() - ref).abs())
    return _entry(ref, e, terms64.abs().sum(0), F32, 'reduction')


def ln_yard(case, dtype):
    inp = ln_inputs(case, dtype)
    x, dy, gamma, beta, eps = inp['x'], inp['dy'], inp['gamma'], inp['beta'], case['eps']
    y, mean, rstd = ln_fwd_ref(x, gamma, beta, eps)
    b = ln_bwd_ref(x, dy, gamma, eps, inp['dy2'], inp['dres'], inp['rscale'], LN_RPG, dtype)
    f = lambda t: None if t is None else t.float()          # noqa: E731
    st = ln_fp32(x.float(), gamma, beta, eps, dy.float(), f(inp['dy2']), f(inp['dres']))
    ms, rs = ln_stat_scales(x, rstd)
    en = dict(y=_entry(y, group_err(st['y'], y, 1), group_max(y, 1), dtype),
              mean=_entry(mean, group_err(st['mean'], mean, None), ms, F32),
              rstd=_entry(rstd, group_err(st['rstd'], rstd, None), rs, F32),
              dx=_entry(b['dx'], group_err(st['dx'], b['dx'], 1), group_max(b['dx'], 1), dtype),
              dgamma=_sum_entry(b['terms_g'], st['g'] * st['xhat'], (st['dgamma'],)),
              dbeta=_sum_entry(b['terms_b'], st['g'], (st['dbeta'],)))
    if DERIVED:
        en['dx']['floor'] = LN_DX_FLOOR
        g = dy if inp['dy2'] is None else dy + inp['dy2']
        if case['cls'] == 'offset':
            en['y']['extra'], en['dx']['extra'], en['dgamma']['extra'] = ln_offset_terms(x, g, gamma, mean, rstd)
        if case['cls'] == 'outlier':
            en['dgamma']['floor'] = ln_dgamma_roundings(case['rows'], case['C'])
    return Yard(case=case, dtype=dtype, inp=inp, entries=en)


def ln_mean_roundings(C):
    """Roundings on the way from a row's elements to its mean in ln_fwd_kernel: a lane adds its 8 * VPT elements one after the other, the
    2^lpr_log2 lanes of a row are added pairwise (wave_sum), the sum is multiplied by the rounded 1 / C."""
    nchunk, lpr_log2 = C // 8, 0
    while (1 << lpr_log2) < nchunk and lpr_log2 < 6:
        lpr_log2 += 1
    vpt = -(-nchunk // (1 << lpr_log2))
    return 8 * vpt + lpr_log2 + 2


# DERIVED floor of dx, every case.  The issue's 4 is the size of two or three roundings of the largest element; dx = rstd (gy - m1 - xhat m2)
# (+ dres) passes through eight on its own way, each at most 2^-24 of a value of the size of the row's largest element: xhat (the difference
# and the product: 2), gy (1), gy - m1 (1), xhat m2 (1), their difference (1), the product with rstd (1), + dres or the rstd that the forward
# stored (1).  The plain two-pass fp32 statement on the CPU needs 4.2 on one element of the tables (test_plain_fp32_layernorm_dx_floor).
LN_DX_FLOOR = 8.0


def ln_dgamma_roundings(rows, C):
    """DERIVED floor of dgamma in the `outlier` class, where ONE term (the outlier's dy * xhat, xhat = 6 or 22) carries a column's sum: every
    rounding on the way then acts on the whole result instead of averaging out over the terms, and the rounding of rstd, which scales
    every xhat the same way, does not average out either.  The count, from ln_fwd_kernel / ln_bwd_kernel: rstd = the variance's sum (the
    mean's chain; the root halves it) + eps, rsqrt (2); xhat (2); the fma into the lane's accumulator, once per row pass; the row lanes of
    the wave (shuffles), the 4 waves (LDS), every 16th block partial and the 16 slices (colreduce_finalize_kernel)."""
    nchunk, lpr_log2 = C // 8, 0
    while (1 << lpr_log2) < nchunk and lpr_log2 < 6:
        lpr_log2 += 1
    rows_per_block = 4 * (64 >> lpr_log2)
    b4 = -(-rows // (rows_per_block * 4))
    blocks = min(-(-rows // rows_per_block) if b4 < 256 else b4, 1024)
    passes = -(-rows // (blocks * rows_per_block))
    return ln_mean_roundings(C) / 2 + 2 + 2 + passes + (6 - lpr_log2) + 4 + -(-blocks // 16) + 16


def ln_offset_terms(x, dy, gamma, mean, rstd):
    """DERIVED term of the `offset` class (mean / sigma = 100), added to the slack of y and dx.
    Why e_ref cannot carry it: F.layer_norm on the CPU updates a running mean (Welford), whose error scales with |x - mean|; the kernel --
    'two-pass statistics in registers (mean, then centred variance), fp32' -- ADDS the elements, so its mean carries the rounding of sums
    of size sum |x|.  Any fp32 sum-then-scale mean does: the plain fp32 statement `ln_manual32` misses the issue's margin on this class
    by a factor of 20 on the CPU, with no kernel involved (test_plain_two_pass_fp32_needs_the_offset_term).
    The term: every element passes through at most R = ln_mean_roundings(C) roundings, each at most 2^-24 of a partial sum <= sum |x|:
        |d mean| <= R 2^-24 mean|x|.
    y = (x - mean) rstd gamma + beta                   ->  |dy_j|  <= |d mean| rstd |gamma_j|
    dx = rstd (gy - m1 - xhat m2), m2 = mean(gy xhat)  ->  |ddx_j| <= rstd (|m2| + |xhat_j| mean|gy|) |d mean| rstd
    dgamma = sum_r g xhat                              ->  |ddgamma_c| <= sum_r |g_rc| |d mean_r| rstd_r
    (d xhat = d mean * rstd enters dx through xhat_j m2 and through m2; the variance changes by (d mean)^2 only).  `dy` is g = dy + dy2."""
    d_mean = ln_mean_roundings(x.shape[1]) * U24 * x.abs().mean(-1, keepdim=True)
    rs = rstd[:, None]
    xh = (x - mean[:, None]) * rs
    gy = dy * gamma.double()
    m2 = (gy * xh).mean(-1, keepdim=True)
    return (d_mean * rs * gamma.double().abs(), rs * (m2.abs() + xh.abs() * gy.abs().mean(-1, keepdim=True)) * d_mean * rs,
            (dy.abs() * d_mean * rs).sum(0))


def ln_judge(Y, got, only=None):
    v = judge(Y.entries, got, f'{Y.case["id"]} {Y.dtype}', only)
    if got.get('dxs') is not None and (only is None or 'dxs' in only):
        # the second output is a function of the STORED dx: the reference takes the dx that was written
        stored = got['dx'].detach().cpu()
        ref = scaled_from_stored(stored.double(), Y.inp['rscale'], LN_RPG)
        sc = Y.inp['rscale'][torch.arange(stored.shape[0]) // LN_RPG][:, None]
        v['dxs'] = compare(got['dxs'], ref, group_err(stored.float() * sc, ref, 1), group_max(ref, 1), Y.dtype, 'elementwise',
                           f'{Y.case["id"]} {Y.dtype} dxs')
    return v


def bn_yard(case, dtype):
    inp = bn_inputs(case, dtype)
    x = inp['x']
    ref = bn_stats_ref(x, BN_EPS, inp['rmean0'], inp['rvar0'], BN_MOMENTUM)
    sts = bn_stats_fp32(x.float(), BN_EPS, inp['rmean0'], inp['rvar0'], BN_MOMENTUM)
    scales = list(bn_stat_scales(x, ref))
    scales[2] = (1 - BN_MOMENTUM) * inp['rmean0'].double().abs() + BN_MOMENTUM * scales[0]        # the sizes of what is added, not of what is left
    en = {}
    for i, name in enumerate(('mean', 'rstd', 'rmean', 'rvar')):
        e = torch.maximum((sts[0][i].double() - ref[i]).abs(), (sts[1][i].double() - ref[i]).abs())
        en[name] = _entry(ref[i], e, scales[i], F32)
    # the running mean carries the mean's error times the momentum (the statement's last rounding may hide its own by chance)
    en['rmean']['e'] = torch.maximum(en['rmean']['e'], BN_MOMENTUM * en['mean']['e'])
    if DERIVED and (case['cls'] in ('offset8', 'offset30', 'outlier') or case['rows'] <= 2):
        en['rstd']['extra'], en['rvar']['extra'] = bn_variance_terms(x, ref[1], case)
    if DERIVED and case['cls'] in ('offset8', 'offset30', 'outlier'):
        # DERIVED floor of the mean (and of the running mean, whose scale holds momentum * mean|x|) where the terms have one sign or one term
        # carries the sum: the partial sums are then as large as the result and nothing averages out, so the floor is the number of
        # roundings on the way, |d S1| <= cr_roundings 2^-24 sum |x|.  (150 rows x 19 channels: 85 row lanes added one after the other.)
        en['mean']['floor'] = en['rmean']['floor'] = cr_roundings(case['rows'], case['C'])
    return Yard(case=case, dtype=dtype, inp=inp, entries=en, statement_stats=(sts[0][0], sts[0][1]),
                given=(torch.zeros(case['C']), torch.ones(case['C'])) if case['cls'] == 'lattice' else None)


def bn_variance_terms(x, rstd, case):
    """DERIVED terms of rstd and the running variance where mean^2 is large against the variance (`offset8`, `offset30`: 64 and 900 times;
    two rows: whenever the two values of a channel happen to be close) or one term carries the sum of squares (`outlier`), added to the slack.  This is the stated contract of segf_bn_stats
    (include/segfac.h): the variance is E[x^2] - mean^2 from fp32 sums, as accurate as those sums allow and no more.  e_ref is the same
    algorithm, but ONE sample of its error per channel: over 2304 channels both summation orders of the statement come out 100 times
    better than typical on some channel, and 4 * e_ref is then no bound for an honest sum.  The a-priori bound, first order:
        |d S1| <= R 2^-24 sum |x|,  |d S2| <= (R + 1) 2^-24 sum x^2   (R = cr_roundings; + 1: the square)
        |d var| <= (R + 1) 2^-24 (E[x^2] + 2 |mean| E|x|),   |d rstd| <= rstd^3 |d var| / 2,   |d running_var| <= momentum n / (n - 1) |d var|."""
    n = x.shape[0]
    dv = (cr_roundings(n, case['C']) + 1) * U24 * ((x * x).mean(0) + 2 * x.mean(0).abs() * x.abs().mean(0))
    return 0.5 * rstd ** 3 * dv, BN_MOMENTUM * (n / (n - 1) if n > 1 else 1.0) * dv


def bn_apply_affine_term(mean32, rstd32, gamma, chan_scale, pre=None, beta=None):
    """DERIVED term of y, every case.  bn_apply_kernel evaluates y = act(a x + b) with a = gamma rstd and b = beta - mean a held in registers
    (one fma per element), not gamma (x - mean) rstd + beta.  Rounding mean * a and then b costs up to 2^-24 (|mean a| + |b|), and
    |b| <= |beta| + |mean a|: beside the roundings of values of the size of y, 2 * 2^-24 |mean gamma rstd| -- next to nothing on friendly
    inputs, 2^-23 * 1600 |gamma| on a constant channel of value 5 (rstd = 316).
    With an activation (pre given) the values of the size of y are not enough either: a channel that ReLU switches off almost everywhere has a
    largest |y| far below its pre-activations, whose roundings (the fma, b, and a's, which acts on pre - beta) stay:  + 2 * 2^-24 (|pre| + |beta|)."""
    t = 2 * U24 * (mean32.double() * gamma.double() * rstd32.double()).abs()[None, :]
    if pre is not None:
        t = t + 2 * U24 * (pre.abs() + beta.double().abs())
    return t if chan_scale is None else t * chan_scale.double().amax(0, keepdim=True)


def bn_dx_cancellation_term(r, x, mean32, rstd32, gamma, n, R):
    """DERIVED term of the training dx in the `outlier` class and at one or two rows, added to the slack.  dx = gamma rstd (d - k1 - xhat k2),
    k1 = sum d / n, k2 = sum d xhat / n: at the outlier (xhat^2 = n - 1) and for any two rows (xhat = +-1) the three terms cancel to a
    10^-5 of their size or less, so the largest |dx| of the channel says nothing about the roundings.  They are bounded by the sizes of
    what is added: d, xhat and the products (5 roundings of the element's own terms), and the sums behind k1 and k2 (R = cr_roundings, + 2:
    the product with 1 / n):   |ddx| <= 2^-24 |gamma rstd| (5 (|d| + |k1| + |xhat k2|) + (R + 2) (sum|d| + |xhat| sum|d xhat|) / n)."""
    xh = (x - mean32.double()) * rstd32.double()
    d, dxh = r['terms_b'], r['terms_g']
    k1, k2 = d.sum(0) / n, dxh.sum(0) / n
    own = d.abs() + k1.abs() + (xh * k2).abs()
    sums = (d.abs().sum(0) + xh.abs() * dxh.abs().sum(0)) / n
    return U24 * (gamma.double() * rstd32.double()).abs() * (5 * own + (R + 2) * sums)


def bn_apply_bwd_entries(Y, mean32, rstd32):
    """Entries of y and of both backward modes for GIVEN fp32 statistics (the ones the statistics step wrote): segf_bn_apply and
    segf_bn_bwd are functions of mean / rstd, and the accuracy of the statistics has its own check.
    ReLU / ReLU6 kinks: the elements of `kink_zone` are left out of the dx comparison, and their dy * xhat (and dy) terms have no part in
    e_ref and scale of dgamma (dbeta) -- the sums themselves keep them, with float64's side of the kink."""
    inp, case, dtype = Y.inp, Y.case, Y.dtype
    x, dy, gamma, beta, cs = inp['x'], inp['dy'], inp['gamma'], inp['beta'], inp['chan_scale']
    act, rps = case['act'], max(case['rps'], 1)
    mean32, rstd32 = mean32.detach().cpu().float(), rstd32.detach().cpu().float()
    y, pre = bn_apply_ref(x, mean32, rstd32, gamma, beta, act, cs, rps)
    y32, _ = bn_apply_ref(x.float(), mean32, rstd32, gamma, beta, act, cs, rps)
    en = dict(y=_entry(y, group_err(y32, y, 0), group_max(y, 0), dtype))
    R = cr_roundings(x.shape[0], case['C'])
    if DERIVED:
        en['y']['extra'] = bn_apply_affine_term(mean32, rstd32, gamma, cs, *((pre, beta) if act else ()))
    keep = ~kink_zone(pre, act)
    for mode in (False, True):
        r = bn_bwd_ref(x, dy, mean32, rstd32, gamma, beta, act, cs, rps, mode)
        s = bn_bwd_ref(x.float(), dy.float(), mean32, rstd32, gamma, beta, act, cs, rps, mode)
        k64, k32 = keep.double(), keep.float()
        e_dx = ((s['dx'].double() - r['dx']).abs() * k64).amax(0, keepdim=True)
        m = 'eval' if mode else 'train'
        en[m] = dict(dx=_entry(r['dx'], e_dx, (r['dx'].abs() * k64).amax(0, keepdim=True), dtype, keep=keep),
                     dgamma=_entry(r['dgamma'], sums_err(s['terms_g'] * k32, (r['terms_g'] * k64).sum(0)), (r['terms_g'] * k64).abs().sum(0),
                                   F32, 'reduction'),
                     dbeta=_entry(r['dbeta'], sums_err(s['terms_b'] * k32, (r['terms_b'] * k64).sum(0)), (r['terms_b'] * k64).abs().sum(0),
                                  F32, 'reduction'))
        if DERIVED and not mode and (case['cls'] == 'outlier' or x.shape[0] <= 2):
            en[m]['dx']['extra'] = bn_dx_cancellation_term(r, x, mean32, rstd32, gamma, x.shape[0], R)
        if DERIVED and case['cls'] == 'outlier':
            # DERIVED floor: one term (the outlier's d * xhat, xhat = 37 to 64) carries the column's sum, so every rounding on its way through
            # the reduction acts on the whole result: the two of xhat, the product, and the chain of cr_roundings
            en[m]['dgamma']['floor'] = R + 3
    return en, pre


def bn_judge(Y, got, only=None):
    """got: mean, rstd, rmean, rvar, y, train = dict(dx, dgamma, dbeta), eval = dict(...)."""
    what = f'{Y.case["id"]} {Y.dtype}'
    v = {} if Y.given is not None else judge(Y.entries, got, what, only)
    en, _ = bn_apply_bwd_entries(Y, *(Y.given if Y.given is not None else (got['mean'], got['rstd'])))
    v.update(judge({'y': en['y']}, got, what, only))
    for m in ('train', 'eval'):
        if got.get(m) is not None:
            v.update({f'{m}.{k}': w for k, w in judge(en[m], got[m], f'{what} {m}', None).items() if only is None or f'{m}.{k}' in only})
    return v


def grn_yard(case, dtype):
    inp = grn_inputs(case, dtype)
    x, dy, gamma, beta, pg = inp['x'], inp['dy'], inp['gamma'], inp['beta'], case['pre_gelu']
    B, C = GRN_B, case['C']
    y, sq, terms_sq = grn_fwd_ref(x, gamma, beta, B, pg)
    b = grn_bwd_ref(x, dy, gamma, B, pg)
    st = grn_fp32(x.float(), gamma, beta, B, pg, dy.float())
    mn = grn_manual32(inp, case, F32)
    per = lambda t: t.reshape(B, -1, C)                       # noqa: E731
    unper = lambda t: t.expand(B, case['rps'], C).reshape(-1, C)     # noqa: E731
    e_sq = torch.stack([sums_err(mn['terms_sq'][i], sq[i]) for i in range(B)])
    # dgamma's terms: Nx[b][c] * dy * a, over every row of every image
    a64 = (gelu64(x) if pg else x)
    G = torch.sqrt(sq)
    Nx = G / (G.mean(-1, keepdim=True) + GRN_EPS)
    terms_g = unper(Nx[:, None]) * dy * a64
    en = dict(y=_entry(y, unper(group_err(per(st['y']), per(y), 1)), unper(group_max(per(y), 1)), dtype),
              sq=_entry(sq, e_sq, sq, F32, 'reduction'),
              dx=_entry(b['dx'], unper(group_err(per(st['dx']), per(b['dx']), 1)), unper(group_max(per(b['dx']), 1)), dtype),
              dgamma=_sum_entry(terms_g, mn['terms_g'], (st['dgamma'],)),
              dbeta=_sum_entry(dy, dy.float(), (st['dbeta'],)))
    if case['rps'] == 1 and DERIVED:
        en['dx']['extra'] = grn_single_row_term(x, dy, gamma, B, pg)
        # ... and of y = (1 + gamma Nx) a + beta, where 1 + gamma Nx and the sum with beta cancel in the same way (gamma Nx = -0.8 gives a
        # coefficient of 0.2 with five times the relative error of Nx): R 2^-24 (|a| + |gamma| Nx |a| + |beta|), + the activation's error
        mag = (1 + gamma.double().abs() * Nx).reshape(B, 1, C) * per(a64).abs() + beta.double().abs()
        en['y']['extra'] = (GRN_SINGLE_ROW_ROUNDINGS * U24 * mag + (GELU_ERR * (1 + gamma.double().abs() * Nx).reshape(B, 1, C) * per(x).abs() if pg else 0)).reshape(-1, C)
    if pg and DERIVED:
        en['sq']['extra'], en['dgamma']['extra'] = grn_gelu_terms(x, dy, gamma, B)
    return Yard(case=case, dtype=dtype, inp=inp, entries=en)


GRN_SINGLE_ROW_ROUNDINGS = 16


def grn_single_row_term(x, dy, gamma, B, pre_gelu):
    """DERIVED term of the one-row images (rows_per_sample = 1), added to the slack of dx.
    There a group (image, channel) is ONE element, so e_ref is one sample of torch's error (often next to 0) and scale is |dx| itself, while
    dx = a dy + K x is a difference of two terms that may each be many times larger -- and K = dG / G, dG = A / m - sum(A G) / (C m^2), is a
    difference as well.  The literal fp32 module with autograd misses the issue's margin against the step-by-step fp32 statement and the
    other way round (factor 18 on the CPU, no kernel involved: test_plain_fp32_grn_needs_the_single_row_term).
    The term bounds the roundings by the sizes of what is added, not of what is left:
        M = (1 + |gamma| Nx) |dy| + ((|A| / m + sum|A G| / (C m^2)) / G) |x|,      |ddx| <= R 2^-24 M
    R = 16 roundings on the longest way from the inputs to dx in grn_coef_kernel / grn_apply_kernel at one row: the square and its root (2);
    the mean of Gx: C / 256 <= 1 lane step, 6 wave_sum steps, 2 block steps, the division (10, shared by both terms of dG); + 1e-6, the
    reciprocal, its square or the product with A (3); the subtraction, the division by G, the product with x, the fma (4) -- 19 less the 3
    that the two branches do not share."""
    C = x.shape[1]
    a = (gelu64(x) if pre_gelu else x).reshape(B, -1, C)
    d = dy.reshape(B, -1, C)
    G = torch.sqrt((a * a).sum(1))
    m = G.mean(-1, keepdim=True) + GRN_EPS
    A = gamma.double().abs() * (d * a).abs().sum(1)
    kmag = torch.where(G > 0, (A / m + (A * G).sum(-1, keepdim=True) / (C * m * m)) / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    M = (1 + gamma.double().abs() * G / m)[:, None] * d.abs() + kmag[:, None] * a.abs()
    M = M.reshape(-1, C)
    if pre_gelu:
        M = M * gelu_grad64(x).abs()
    return GRN_SINGLE_ROW_ROUNDINGS * U24 * M


# |d gelu(x)| <= GELU_ERR |x|: half the error of the kernels' erf (gelu = x / 2 (1 + erf)).  erf is Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 by
# its formula, evaluated in fp32 as 1 - p t e: eight roundings of values below 1 (the five of p, t, e, the products), 2^-25 each.  (csrc/common.h
# states 0.8e-7 |x|, the formula's share alone; at |x| = 1e-4 the kernels are at 1.4e-7 |x|.)
GELU_ERR = 0.5 * (1.5e-7 + 8 * 2.0 ** -25)


def grn_gelu_terms(x, dy, gamma, B):
    """DERIVED terms of the two reductions that read gelu(x) (pre_gelu), added to the slack.  The kernels' erf is Abramowitz & Stegun 7.1.26,
    |error| <= 1.5e-7 ABSOLUTE, so |d gelu(x)| <= GELU_ERR |x| (above).  For x < 0 that is far more than 2^-24 gelu(x), F.gelu's own
    error, and the sums of a^2 and of dy a carry it:
        |d sum a^2| <= sum (2 |a| + da) da,   da = GELU_ERR |x|
        dgamma = sum_b Nx_b sum_p dy a:  |d| <= sum_b (Nx sum_p |dy| da + sum_p |dy a| dNx),  dNx <= Nx (dG / G + mean_c dG / m),  dG = d(sum a^2) / (2 G)."""
    C = x.shape[1]
    a = gelu64(x).reshape(B, -1, C)
    da = GELU_ERR * x.abs().reshape(B, -1, C)
    d = dy.reshape(B, -1, C)
    dsq = ((2 * a.abs() + da) * da).sum(1)
    G = torch.sqrt((a * a).sum(1))
    pos = G > 0
    Gs = torch.where(pos, G, torch.ones_like(G))
    m = G.mean(-1, keepdim=True) + GRN_EPS
    dG = torch.where(pos, dsq / (2 * Gs), torch.sqrt(dsq))
    Nx = G / m
    dNx = Nx * (torch.where(pos, dG / Gs, torch.zeros_like(G)) + dG.mean(-1, keepdim=True) / m) + torch.where(pos, torch.zeros_like(G), dG / m)
    return dsq, (Nx * (d.abs() * da).sum(1) + (d * a).abs().sum(1) * dNx).sum(0)


def grn_judge(Y, got, only=None):
    return judge(Y.entries, got, f'{Y.case["id"]} {Y.dtype}', only)


def colsum_yard(case, dtype):
    inp = colsum_inputs(case, dtype)
    en = _sum_entry(inp['x'], inp['x'].float())
    assert torch.equal(en['ref'], colsum_ref(inp['x']))
    return Yard(case=case, dtype=dtype, inp=inp, entries=dict(sum=en))


def colsum_judge(Y, got, only=None):
    return judge(Y.entries, got, f'{Y.case["id"]} {Y.dtype}', only)


OPS = dict(ln=(ln_cases, ln_yard, ln_manual32, ln_judge), bn=(bn_cases, bn_yard, bn_manual32, bn_judge),
           grn=(grn_cases, grn_yard, grn_manual32, grn_judge), colsum=(colsum_cases, colsum_yard, colsum_manual32, colsum_judge))

# name -> (operation, the wrong computation's tag in the *_manual32 functions, substrings that select the cases it is tried on, the outputs
# that may reject it).  Every one is an error of at least 1e-3 of the output on the right input class and next to nothing on `plain`.
MUTANTS = {
    'eps outside the square root': [('ln', 'eps_outside', ('ln-tiny-333x40', 'ln-const-333x40'), ('y', 'rstd')),
                                    ('bn', 'eps_outside', ('bn-tiny-150x19', 'bn-const-150x19'), ('rstd',))],
    'eps dropped': [('ln', 'eps_dropped', ('ln-tiny-333x40', 'ln-const-333x40'), ('y', 'rstd')),
                    ('bn', 'eps_dropped', ('bn-tiny-150x19', 'bn-const-150x19'), ('rstd',))],
    'mean divided by C rounded up to the lane width': [('ln', 'mean_padded_width', ('ln-offset-333x40', 'ln-plain-37x24'), ('mean', 'y'))],
    'biased variance in the running statistics': [('bn', 'running_biased', ('bn-plain-2x72', 'bn-plain-150x19'), ('rvar',))],
    'unbiased variance in rstd': [('bn', 'rstd_unbiased', ('bn-plain-2x72', 'bn-plain-150x19'), ('rstd',))],
    'last row dropped': [('colsum', 'last_row_dropped', ('colsum-positive-4101x72', 'colsum-alternating-4101x72'), ('sum',)),
                         ('bn', 'last_row_dropped', ('bn-offset8-4101x72-act1',), ('mean',)),
                         ('ln', 'last_row_dropped', ('ln-plain-4101x512',), ('dgamma', 'dbeta'))],
    'last row counted twice': [('colsum', 'last_row_twice', ('colsum-positive-4101x72', 'colsum-alternating-4101x72'), ('sum',)),
                               ('bn', 'last_row_twice', ('bn-offset8-4101x72-act1',), ('mean',)),
                               ('ln', 'last_row_twice', ('ln-plain-4101x512',), ('dgamma', 'dbeta'))],
    'last 8-channel chunk taken from the previous row': [('ln', 'chunk_prev_row', ('ln-plain-333x40', 'ln-plain-9x520'), ('y', 'mean'))],
    'mean rounded to bf16': [('ln', 'mean_bf16', ('ln-offset-333x40',), ('mean', 'y')), ('bn', 'mean_bf16', ('bn-offset30-150x19',), ('mean',))],
    'rstd rounded to bf16': [('ln', 'rstd_bf16', ('ln-plain-333x40',), ('rstd', 'y')), ('bn', 'rstd_bf16', ('bn-plain-150x19',), ('rstd',))],
    'dgamma from x - mean without * rstd': [('ln', 'dgamma_no_rstd', ('ln-plain-333x40', 'ln-big-333x40'), ('dgamma',))],
    'dy2 ignored': [('ln', 'dy2_ignored', ('ln-fanin',), ('dx', 'dgamma', 'dbeta'))],
    'dres added before the rstd factor': [('ln', 'dres_before_rstd', ('ln-fanin',), ('dx',))],
    'dxs scaled from the unrounded dx': [('ln', 'dxs_unrounded', ('ln-fanin',), ('dxs',))],
    'rows_per_sample off by one in chan_scale': [('bn', 'rps_off_by_one', ('bn-plain-150x19', 'bn-plain-4101x72-act1'), ('y',))],
    'ReLU6 mask closed at 6 the wrong way': [('bn', 'relu6_closed_at_6', ('bn-lattice-150x24-act2',), ('train.dx', 'eval.dx'))],
    'GRN without its eps on an all-zero image': [('grn', 'eps_dropped', ('grn-zero_image-49x40',), ('y', 'dx'))],
    'GRN mean of Gx over C - 1': [('grn', 'mean_over_c_minus_1', ('grn-plain-49x40', 'grn-plain-1x8'), ('y',))],
    'GRN K not zeroed for a zero channel': [('grn', 'k_not_zeroed', ('grn-zero_channel-49x40',), ('dx',))],
    'colsum with one partial rounded to bf16': [('colsum', 'partial_bf16', ('colsum-positive-4101x72', 'colsum-offset-4101x72'), ('sum',))],
}
BF16_ONLY_MUTANTS = ('dxs_unrounded',)          # the two roundings coincide in fp32 storage
