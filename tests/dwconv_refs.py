"""Float64 statements of the depthwise 3 x 3 (+ bias, + GELU) and 7 x 7 (+ bias) convolutions on NHWC maps and of their backward passes, the
per-element bounds of tests/test_dwconv_float64.py, the case tables its GPU tests run, and mutants of the statements.  Importable without a
GPU.  The operations are those of include/segfac.h, written as sums over shifted slices of a zero-padded [B][H][W][C] tensor -- no
F.conv2d, no transcription of a kernel:

    t  = b + sum_k w_k x[p + off_k]                 k = (ky, kx), off_k = (ky - r, kx - r), r = 1 or 3
    y  = gelu(t)  or  t
    du = dy * gelu'(t)  or  dy
    dx = sum_k w_k du[p - off_k]
    dw[c][k] = sum_p du[p] x[p + off_k],    db[c] = sum_p du[p]

Activations enter ALREADY ROUNDED to the storage type (norm_refs.to_storage), as float64; weights and bias are fp32 values.

Bounds (u = 2^-24, n = k * k taps; every one per element, none a share of the tensor's largest element; `compare` of norm_refs with the
bound as its `extra` term and margin 1, so the printed ratio is (err - half_ulp) / bound and must stay at or below 1):

  y without GELU    half_ulp_T(y64) + n u A_t,  A_t = |b| + sum_k |w_k x_k|: an fp32 multiply-add chain over n terms that starts from the
                    bias rounds n times, each time a partial sum of size <= A_t, in any order.
  y with GELU       half_ulp_T(y64) + G1 n u A_t + GELU_ERR |t64|: the error of t through the largest slope of gelu, and the absolute
                    error of the kernels' erf (norm_refs.GELU_ERR).  DERIVED, every case: + GELU_CHAIN_TERM |t64|, the roundings of the
                    erf polynomial that GELU_ERR's count leaves out (below).
  du                half_ulp_T(du64) + |dy| (G2 n u A_t + GELU_GRAD_ERR): the error of t through the largest slope of gelu', and the
                    absolute error of gelu_erf8<true> per unit of dy (below).
  dx, du in memory  pass C is a function of what pass A WROTE: dx64' = convT(du_got), half_ulp_T(dx64') + n u sum_k |w_k du_got_k|.
  dx, du not kept   (the one-launch form)  half_ulp_T(dx64) + sum_k |w_k| d_k + n u A_dx, A_dx = sum_k |w_k du64_k|.  Derivation: the kernel
                    computes fl(sum_k w_k du'_k) with du' = du64 + delta, |delta| <= d (the du bound at the tap's pixel, which holds the half
                    ulp of du's rounding to T in LDS); sum_k w_k delta_k <= sum_k |w_k| d_k, and the chain's own roundings are
                    n u sum_k |w_k du'_k| = n u A_dx to first order (the difference, n u sum |w_k| d_k, is second order).
  dw, db            norm_refs.CLASSES['reduction'] (MARGIN 2, FLOOR 4): max(2 e_ref, 4 u scale), scale = the float64 sum of the absolute
                    terms, e_ref = the larger error of torch's `.sum(0)` and of the sequential fp32 sum (norm_refs.sums_err) of the fp32
                    terms formed on the CPU from the same du: du_got where the call leaves it in memory, else du64 rounded to T plus the
                    term sum_p d[p] |x[p + off_k]| (db: sum_p d[p]).
"""
import functools
import math

import torch
import torch.nn.functional as F

import exact_inputs as X
import norm_refs as R
from norm_refs import BF, F32, F64, GELU_ERR, U24, gelu64, gelu_grad64, half_ulp, seed_of, to_storage

DERIVED = True                         # False: the issue's bound alone, without the derived terms of single cases (for measurements)
# DERIVED term of every multiply-add chain (t, dx), every case: n 2^-149.  The relative model fl(a b + c) = (a b + c)(1 + delta), |delta| <= u,
# holds for normal results only; a result below 2^-126 lies on the denormal grid of spacing 2^-149, whatever its size, so each of the n
# roundings may cost up to that much instead.  It shows where du underflows: behind a saturated GELU (class `big`) gelu'(-13) = 1e-36 and
# dx is a sum of denormals -- 6.4e-40 against a relative bound of 3.4e-46, a fifth of the grid.
UNDERFLOW = 2.0 ** -149

# G1 = max |gelu'|: gelu'(x) = Phi(x) + x phi(x), gelu''(x) = (2 - x^2) phi(x) = 0 at x = sqrt 2, where gelu' = Phi(sqrt 2) + sqrt 2 phi(sqrt 2)
G1 = 0.5 * (1 + math.erf(1.0)) + math.sqrt(2.0) * math.exp(-1.0) / math.sqrt(2 * math.pi)          # 1.12890
# G2 = max |gelu''|: (gelu'')' = x (x^2 - 4) phi(x) = 0 at x = 0 and |x| = 2; |gelu''(0)| = 2 phi(0) = 0.798 > |gelu''(2)| = 2 phi(2) = 0.108
G2 = 2.0 / math.sqrt(2 * math.pi)
# The roundings of the kernels' erf = 1 - P(t) e, P(t) = t p(t) (Abramowitz & Stegun 7.1.26 on t = 1 / (1 + 0.2316 |x|), e = exp2(x x (-log2(e) / 2)),
# csrc/common.h gelu_erf8), in units of 2^-24, each fused multiply-add rounding once:
#   t         a value in (0, 1], half a unit 2^-25, through the slope of P: P'(t) <= P'(1) = 3.444 on (0, 1]                   1.72
#   p         four multiply-adds whose values reach 1.45 (the coefficients), 2^-24 each, times powers of t <= 1               4
#   p t       a value below P(1) < 1                                                                                           0.5
#   e         exp2, one unit of a value below 1, times P <= 1                                                                  1
#   1 - p t e a value in [0, 1]                                                                                                0.5
# norm_refs.GELU_ERR counts 'eight roundings of values below 1, 2^-25 each' = 4 of these 7.72 units: it leaves out the slope of P and that the
# intermediate values of p exceed 1.  test_gelu_emulation_* shows it on the CPU: the formula evaluated step by step in fp32 is at
# 1.44 GELU_ERR |x| near |x| = 0.06.
ERF_ROUNDINGS = 3.444 / 2 + 4 + 0.5 + 1 + 0.5
# DERIVED term of y with GELU, every case, added to GELU_ERR |t|: half of the roundings that GELU_ERR leaves out (gelu = x / 2 (1 + erf)), and
# the last multiply-add h erf + h, one rounding of a value |gelu| <= |x| that an fp32 store does not pay again (half_ulp_T is 0 there).
GELU_CHAIN_TERM = 0.5 * (ERF_ROUNDINGS * U24 - 8 * 2.0 ** -25) + U24
# |d (dy gelu'(x))| <= GELU_GRAD_ERR |dy|, ABSOLUTE in gelu': gelu_erf8<true> evaluates dy (x e c + (erf / 2 + 1 / 2)), c = 1 / sqrt(2 pi).
#   erf / 2                   half of the formula's 1.5e-7 and of the roundings above                                  0.5 (1.5e-7 + 7.72 2^-24)
#   erf / 2 + 1 / 2           one multiply-add, a value in [0, 1]                                                      2^-25
#   x e                       a value <= e^-1/2 = 0.61                                                                 2^-25
#   (x e) c + cdf             one multiply-add, a value <= G1 < 2                                                      2^-24
#   the product with dy       one rounding of a value <= G1 |dy|                                                       G1 2^-24
#   exp2's argument           q = x x (-log2(e) / 2): two roundings and the constant's, |dq| <= 2.5 2^-24 |q|, and exp2's own unit where e
#                             enters a second time: |de| <= (2.5 s + 2) 2^-24 e^-s with s = x^2 / 2.  Through x e c: c |x| (2.5 s + 2) e^-s
#                             <= c (2.5 * 0.58 + 2 * 0.61) = 1.07 (|x| s e^-s <= 0.58, at x = sqrt 3); through erf / 2 (P <= 1), the
#                             argument's share: 2.5 / e / 2 = 0.46                                                     1.53 2^-24
GELU_GRAD_ERR = 0.5 * (1.5e-7 + ERF_ROUNDINGS * U24) + 2.0 ** -25 + 2.0 ** -25 + U24 + G1 * U24 + 1.53 * U24


def _fma(a, b, c):
    """fp32 a * b + c with ONE rounding (the product of two fp32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def gelu_erf8_emulated(x32, grad):
    """gelu_erf8<GRAD> of csrc/common.h step by step in torch fp32, operation for operation: a product followed by a sum is one fused
    multiply-add, as the compiler contracts it.  grad: gelu'(x) (the factor of dy), else gelu(x)."""
    f = lambda v: torch.tensor(v, dtype=F32)                  # noqa: E731
    x = x32.to(F32)
    q = x * x * f(-0.72134752044448170368)
    d = _fma(x.abs(), f(0.3275911) * f(0.70710678118654752440), f(1.0))
    e, t = torch.exp2(q), f(1.0) / d
    p = _fma(t, f(1.061405429), f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, f(c))
    er = torch.copysign(_fma(-(p * t), e, f(1.0)), x)
    if grad:
        return _fma(x * e, f(0.39894228040143267794), _fma(er, f(0.5), f(0.5)))
    h = x * f(0.5)
    return _fma(h, er, h)


def gelu_tanh64(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_tanh_grad64(x):
    a = math.sqrt(2 / math.pi)
    th = torch.tanh(a * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * a * (1 + 3 * 0.044715 * x * x)


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def taps(k):
    return [(ky, kx) for ky in range(k) for kx in range(k)]


class Shifted:
    """t[p + sign * off_k] of a [B][H][W][C] tensor, zero outside the map."""

    def __init__(self, t4, k):
        self.r, (_, self.H, self.W, _) = k // 2, t4.shape
        self.p = F.pad(t4, (0, 0, self.r, self.r, self.r, self.r))

    def __call__(self, ky, kx, sign=1):
        r = self.r
        oy, ox = r + sign * (ky - r), r + sign * (kx - r)
        return self.p[:, oy:oy + self.H, ox:ox + self.W]


def _wk(w, i):
    return w.double()[:, i]                                    # [C]: broadcasts over [B][H][W][C]


def conv_ref(x, w, b, k, sign=1, mut=None):
    """(b + sum_k w_k x[p + sign off_k], |b| + sum_k |w_k x[p + sign off_k]|).  sign = -1: the transposed convolution of the backward.
    mut 'tap_dropped_last_col': the pixels of the last column lose the tap to their left when W % 4 != 0."""
    sh = Shifted(x, k)
    s = torch.zeros_like(x) if b is None else b.double().expand_as(x).clone()
    a = s.abs()
    for i, (ky, kx) in enumerate(taps(k)):
        term = _wk(w, i) * sh(ky, kx, sign)
        if mut == 'tap_dropped_last_col' and x.shape[2] % 4 != 0 and (ky, kx) == (k // 2, k // 2 - 1):
            term = term.clone()
            term[:, :, -1] = 0
        s = s + term
        a = a + term.abs()
    return s, a


def fwd_ref(x, w, b, k, gelu, mut=None):
    """-> dict(t, y, A_t)."""
    t, A = conv_ref(x, w, b, k, 1, mut)
    y = (gelu_tanh64(t) if mut == 'tanh_gelu' else gelu64(t)) if gelu else t
    return dict(t=t, y=y, A_t=A)


def du_ref(t, dy, gelu, b=None, mut=None):
    if not gelu:
        return dy.clone()
    if mut == 'bias_left_out_bwd' and b is not None:
        t = t - b.double()
    return dy * (gelu_tanh_grad64(t) if mut == 'tanh_gelu' else gelu_grad64(t))


def wgrad_ref(x, du, k, mut=None, seam_row=None):
    """-> (dw [C][k k], db [C], sum_p |du x| [C][k k], sum_p |du| [C]).  mut 'seam_row_twice': image row `seam_row` counted twice in dw."""
    sh = Shifted(x, k)
    dw, sa = [], []
    for ky, kx in taps(k):
        term = du * sh(ky, kx)
        s = term.sum((0, 1, 2))
        if mut == 'seam_row_twice':
            s = s + term[:, seam_row].sum((0, 1))
        dw.append(s)
        sa.append(term.abs().sum((0, 1, 2)))
    return torch.stack(dw, 1), du.sum((0, 1, 2)), torch.stack(sa, 1), du.abs().sum((0, 1, 2))


def dx_ref(du, w, k, mut=None):
    """-> (dx, A_dx)."""
    return conv_ref(du, w, None, k, 1 if mut == 'kernel_not_flipped' else -1)


# ---- host arithmetic of csrc/conv.hip restated (which form a shape takes; how many partial blocks it leaves) ---------------------------
def small_nch(dtype, B, H, W, C, always=False):
    """dw_small_nch: 8-channel chunks per workgroup of the one-launch form, 0 where the map does not take it."""
    HW, umax = H * W, 1024 if dtype == BF else 512
    if C % 8 or B > 4096 or HW > umax or HW < 16:
        return 0
    for nch in (4, 2, 1):
        if HW * nch <= umax and (C // 8) % nch == 0:
            return nch if (B * (C // (8 * nch)) <= 512 or always) else 0
    return 0


def walk_plan(B, H, W, C, rows=0):
    """dw_walk_plan -> (R, nseg)."""
    columns = B * -(-W // 4) * (C // 4)
    nseg = -(-H // 64)
    while columns * nseg < 131072 and -(-H // nseg) > 8:
        nseg *= 2
    if rows > 0:
        nseg = -(-H // rows)
    return -(-H // nseg), nseg


def wgrad_blocks(form, dtype, B, H, W, C, rows=0):
    """segf_dwconv3x3_bwd_blocks for a forced form: B (one-launch), dwg_plan.nblk (strip), dww_plan.nblk (walk)."""
    if form == 'small':
        return B
    if form == 'strip':
        nchunk = C // 8
        ch = min(nchunk, 256)
        rl, slabs = 256 // ch, -(-nchunk // ch)
        return max(1, min(-(-(B * H * -(-W // 4)) // (rl * 4)), max(1024 // slabs, 1)))
    nchunk, best, pick = C // 4, -1.0, (1, C // 4)
    for sl in range(1, 9):
        ch = -(-nchunk // sl)
        if ch > 256:
            continue
        util = (ch * (256 // ch)) / 256.0 * nchunk / (ch * sl)
        if util > best + 1e-9:
            best, pick = util, (ch, sl)
    ch, slabs = pick
    _, nseg = walk_plan(B, H, W, C, rows)
    return max(1, min(-(-(B * nseg * -(-W // 4)) // (256 // ch)), max(2048 // slabs, 1)))


def wgrad_roundings(form, dtype, B, H, W, C, rows=0):
    """Additions on the longest way of a term of dw / db through the weight-gradient reduction of a form, restating the plans of
    csrc/conv.hip and csrc/colreduce.h: a thread adds the terms of its units one after the other (4 pixels a strip; a walk unit is 4 pixels
    x R rows), the rl unit lanes of a workgroup are added one after the other, the finalize adds every 16th block partial and then its 16
    slices.  One-launch form: a thread adds its contiguous slice of the H W pixels, the S slices are added in order, then the B image
    partials go through the same finalize.  |error of the sum| <= wgrad_roundings * 2^-24 * sum |terms| (first order)."""
    strips = -(-W // 4)
    if form == 'small':
        S = 256 // (10 * small_nch(dtype, B, H, W, C, always=True))
        return -(-(H * W) // S) + S + -(-B // 16) + 16
    nblk = wgrad_blocks(form, dtype, B, H, W, C, rows)
    if form == 'strip':
        ch = min(C // 8, 256)
        rl, units, per_unit = 256 // ch, B * H * strips, 4
    else:
        nchunk, best, ch = C // 4, -1.0, 1
        for sl in range(1, 9):
            c2 = -(-nchunk // sl)
            util = (c2 * (256 // c2)) / 256.0 * nchunk / (c2 * sl) if c2 <= 256 else -2.0
            if util > best + 1e-9:
                best, ch = util, c2
        R_, nseg = walk_plan(B, H, W, C, rows)
        rl, units, per_unit = 256 // ch, B * nseg * strips, 4 * R_
    return per_unit * -(-units // (nblk * rl)) + rl + -(-nblk // 16) + 16


def dw7_strips_per_thread(B, H, W, C):
    """dw7_blocks: strips per thread of dwconv7x7_kernel."""
    units = B * H * -(-W // 8)
    return max(1, min(4, units * (C // 8) // 256 // 2048))


# ---- the case tables --------------------------------------------------------------------------------------------------------------
SHAPES3 = (
    ((1, 1, 1, 8), 'one pixel, every tap but the centre clipped'),
    ((3, 1, 16, 128), 'H = 1'),
    ((2, 2, 5, 24), 'a segment shorter than the walk\'s three-row rotation; W ragged; 3 and 6 chunks against 256 threads'),
    ((2, 3, 5, 40), 'H W = 15, one under the small form\'s lower bound'),
    ((2, 4, 4, 40), 'H W = 16, on the lower bound'),
    ((2, 16, 32, 64), '512 pixels, the fp32 upper bound of the small form'),
    ((2, 32, 32, 64), '1024 pixels, the bf16 upper bound of the small form'),
    ((1, 33, 32, 64), '1056 pixels, over both bounds'),
    ((1, 70, 6, 136), '16 segments of 5 rows for 70 rows: the last segments ragged and empty'),
    ((2, 130, 7, 16), 'W = 7, many seams (rows unset, 3, 64)'),
    ((2, 9, 22, 640), '160 four-channel chunks: dww_plan deals them as five slabs of 32 (eight unit lanes); nch 4 (bf16) / 2 (fp32) in the small form'),
    ((1, 5, 6, 2056), 'strip wgrad: two slabs, one live chunk in the second; walk wgrad: seven slabs of 74, four idle lanes in the last'),
)
CLASSES = ('plain', 'offset', 'big', 'tiny', 'negative', 'sparse', 'nobias')
CLASS_SHAPES = ((2, 9, 22, 640), (2, 2, 5, 24))
ROWS_SHAPE = (2, 130, 7, 16)
SHAPES7 = (
    ((1, 1, 1, 8), 'one pixel'),
    ((2, 3, 5, 24), 'a map smaller than the kernel'),
    ((2, 7, 9, 40), 'two strips, the second with one live pixel'),
    ((1, 9, 17, 96), 'three strips, the last with one live pixel'),
    ((2, 9, 11, 2816), 'two slabs in dw7_plan, 96 live chunks in the second'),
)
FC2_CASES = (((2, 5, 16, 128, 32), 0), ((2, 9, 22, 128, 32), 0), ((2, 9, 22, 128, 32), 3), ((3, 1, 16, 128, 32), 0), ((1, 70, 36, 256, 64), 0))


def _sid(shape):
    return 'x'.join(map(str, shape))


def cases3():
    """[dict(id, k, shape, cls, gelu)]: `plain` on every shape with and without GELU; the other classes on CLASS_SHAPES with GELU (and
    `offset`, whose point is A_t >> |t|, without it too)."""
    out = [dict(id=f'dw3-plain-{_sid(s)}-{"gelu" if gl else "id"}', k=3, shape=s, cls='plain', gelu=gl) for s, _ in SHAPES3 for gl in (True, False)]
    for s in CLASS_SHAPES:
        for cls in CLASSES[1:]:
            for gl in ((True, False) if cls == 'offset' else (True,)):
                out.append(dict(id=f'dw3-{cls}-{_sid(s)}-{"gelu" if gl else "id"}', k=3, shape=s, cls=cls, gelu=gl))
    return out


def cases7():
    """`plain` (with bias) and `nobias` on every shape; `offset` and `sparse` on the map smaller than the kernel and on (2, 7, 9, 40)."""
    out = [dict(id=f'dw7-{cls}-{_sid(s)}', k=7, shape=s, cls=cls, gelu=False) for s, _ in SHAPES7 for cls in ('plain', 'nobias')]
    out += [dict(id=f'dw7-{cls}-{_sid(s)}', k=7, shape=s, cls=cls, gelu=False) for s in ((2, 3, 5, 24), (2, 7, 9, 40)) for cls in ('offset', 'sparse')]
    return out


def forms3(case, dtype, backward):
    """[(form, rows)] a 3 x 3 case runs in: strip, walk (with SEGFAC_DW_WALK_ROWS unset, 3 and 64 on ROWS_SHAPE) and, backward only and
    inside its H W bounds, the one-launch form."""
    B, H, W, C = case['shape']
    out = [('strip', 0), ('walk', 0)]
    if case['shape'] == ROWS_SHAPE:
        out += [('walk', 3), ('walk', 64)]
    if backward and small_nch(dtype, B, H, W, C, always=True):
        out.append(('small', 0))
    return out


FORM_ENV = {'strip': {'SEGFAC_DW_NO_WALK': '1', 'SEGFAC_DW_NO_SMALL': '1'}, 'walk': {'SEGFAC_DW_NO_SMALL': '1'},
            'small': {'SEGFAC_DW_SMALL_ALWAYS': '1'}}
_T = {F32: 'T = float', BF: 'T = unsigned short'}


def form_kernels(form, dtype, backward):
    """What a form must name in the launch trace: a list of tuples of substrings, each tuple to be found together in ONE kernel name."""
    if form == 'strip':
        return [('dwconv3x3_kernel<T, 2>',), ('dwconv3x3_wgrad_kernel<T>',), ('dwconv3x3_kernel<T, 1>',), ('dw_scatter_kernel',)] if backward \
            else [('dwconv3x3_kernel<T, 0>',)]
    if form == 'walk':
        return [('dwconv3x3_walk_kernel<', _T[dtype], 'MODE = 2]'), ('dwconv3x3_wgrad_walk_kernel<T>',),
                ('dwconv3x3_walk_kernel<', _T[dtype], 'MODE = 1]'), ('dw_scatter_kernel',)] if backward \
            else [('dwconv3x3_walk_kernel<', _T[dtype], 'MODE = 0]')]
    assert backward
    return [('dwconv3x3_bwd_small_kernel<T>',), ('dw_scatter_kernel',)]


FORBIDDEN_KERNELS = {'strip': ('walk', 'small'), 'walk': ('dwconv3x3_kernel<', 'dwconv3x3_wgrad_kernel', 'small'),
                     'small': ('dwconv3x3_kernel<', 'walk', 'wgrad')}


SWITCHES = ('SEGFAC_DW_NO_WALK', 'SEGFAC_DW_WALK_ROWS', 'SEGFAC_DW_NO_SMALL', 'SEGFAC_DW_SMALL_ALWAYS', 'SEGFAC_FFN_BWD_FUSED')


def release_forms(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def force_form(monkeypatch, form, rows=0, fused=None):
    """One form of the 3 x 3 through the existing switches (tests/conftest.py re-reads the policy on every change); the rest at its default."""
    release_forms(monkeypatch)
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)
    if rows:
        monkeypatch.setenv('SEGFAC_DW_WALK_ROWS', str(rows))
    if fused is not None:
        monkeypatch.setenv('SEGFAC_FFN_BWD_FUSED', str(fused))


def assert_form_ran(trace, form, dtype, backward):
    """The kernels of the form ran (in a dry run: were chosen), and no depthwise 3 x 3 kernel of another form."""
    assert trace.launches > 0 or trace.kernels, 'no kernel was launched'
    for subs in form_kernels(form, dtype, backward):
        assert any(all(s in k for s in subs) for k in trace.kernels), (form, subs, trace.kernels)
    for s in FORBIDDEN_KERNELS[form]:
        assert not any(s in k for k in trace.kernels if 'dwconv3x3' in k), (form, s, trace.kernels)


def _randn(shape, g):
    return torch.randn(tuple(shape), generator=g, dtype=F32)


def inputs(case, dtype):
    """float64 activations x, dy [B][H][W][C] (rounded to `dtype`), fp32 w [C][k k] and bias [C] (None: class `nobias`).
    plain     x, dy = randn, w = 0.3 randn, b = randn
    offset    x = 8 + randn, every channel's weights sum to zero: A_t >> |t|
    big       x * 2^6: GELU saturated on both sides
    tiny      x and b * 2^-12: the linear region, where only the relative error of gelu' shows
    negative  b = -6: y tiny, the absolute GELU term carries the bound
    sparse    80 % exact zeros in x and in dy, and the last image all zero in both
    nobias    a null bias pointer"""
    g = X.gen(seed_of(case['id']))
    (B, H, W, C), k, cls = case['shape'], case['k'], case['cls']
    x, dy = _randn((B, H, W, C), g), _randn((B, H, W, C), g)
    w, b = 0.3 * _randn((C, k * k), g), _randn((C,), g)
    if cls == 'offset':
        x = x + 8
        w = w - w.mean(1, keepdim=True)
    elif cls == 'big':
        x = x * 64
    elif cls == 'tiny':
        x, b = x * 2.0 ** -12, b * 2.0 ** -12
    elif cls == 'negative':
        b = torch.full((C,), -6.0)
    elif cls == 'sparse':
        x = x * (torch.rand(x.shape, generator=g) < 0.2)
        dy = dy * (torch.rand(x.shape, generator=g) < 0.2)
        x[-1], dy[-1] = 0, 0
    elif cls == 'nobias':
        b = None
    return dict(x=to_storage(x, dtype), dy=to_storage(dy, dtype), w=w, b=b)


def fc2_inputs(shape, rows):
    """The Mix-FFN form (bf16): dys [M][C_in] and w2 [C_in][C_hidden] are lattice values, so dg = dys W2 is an exact integer below 2^24
    whose ONE bf16 rounding is known; x, w9 and bias are random."""
    B, H, W, Cc, Cin = shape
    g = X.gen(seed_of(f'fc2-{_sid(shape)}-{rows}'))
    dys, w2 = X.lattice((B * H * W, Cin), g), X.lattice((Cin, Cc), g)
    dg = dys @ w2
    assert dg.abs().max() < 2 ** 24 and (dg == dg.round()).all()
    return dict(x=to_storage(_randn((B, H, W, Cc), g), BF), dy=X.round_bf16(dg).double().reshape(B, H, W, Cc), w=0.3 * _randn((Cc, 9), g),
                b=_randn((Cc,), g), dys=dys, w2=w2)


# ---- yardsticks and judges --------------------------------------------------------------------------------------------------------
def _bound_entry(ref, bound, store):
    """An elementwise output under a derived per-element bound: |got - ref| <= half_ulp_T(ref) + bound; ratio = (err - half_ulp) / bound."""
    return dict(ref=ref, e=0.0, scale=0.0, store=store, cls='elementwise', keep=None, margin=1.0, floor=0.0, extra=bound)


def _rows(t4):
    return t4.reshape(-1, t4.shape[-1])


def _sum_entries(x, du_terms, k, dtype, extra_d=None):
    """Entries of dw [C][k k] and db [C] for the du the sums were (or must have been) taken over: reference and scale in float64, e_ref
    from the fp32 terms du * x formed on the CPU (norm_refs.sums_err: torch's `.sum(0)` and the sequential fp32 sum)."""
    sh = Shifted(x, k)
    du32 = du_terms.float()
    ref, e, sc, ex = [], [], [], []
    for ky, kx in taps(k):
        xs = sh(ky, kx)
        t64 = _rows(du_terms * xs)
        r = t64.sum(0)
        ref.append(r)
        e.append(R.sums_err(_rows(du32 * xs.float()), r))
        sc.append(t64.abs().sum(0))
        if extra_d is not None:
            ex.append(_rows(extra_d * xs.abs()).sum(0))
    st = lambda v: torch.stack(v, 1)                           # noqa: E731
    dw = dict(ref=st(ref), e=st(e), scale=st(sc), store=F32, cls='reduction', keep=None)
    rb = _rows(du_terms).sum(0)
    db = dict(ref=rb, e=R.sums_err(_rows(du32), rb), scale=_rows(du_terms).abs().sum(0), store=F32, cls='reduction', keep=None)
    if extra_d is not None:
        dw['extra'], db['extra'] = st(ex), _rows(extra_d).sum(0)
    return dw, db


class Yard(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=4)
def _yard_cached(key, dtype):
    case = CASE_BY_ID[key]
    return make_yard(case, inputs(case, dtype), dtype)


def yard(case, dtype):
    """The float64 results of a case and the entries that do not depend on what a kernel wrote (y, du; dx / dw / db of the form that keeps
    no du).  Shared, unchanged, by every form of the case."""
    return _yard_cached(case['id'], dtype)


def make_yard(case, inp, dtype):
    k, gelu = case['k'], case['gelu']
    n = k * k
    x, dy, w, b = inp['x'], inp['dy'], inp['w'], inp['b']
    f = fwd_ref(x, w, b, k, gelu)
    du = du_ref(f['t'], dy, gelu)
    under = n * UNDERFLOW if DERIVED else 0.0
    chain = n * U24 * f['A_t'] + under
    y_bound = G1 * chain + (GELU_ERR + (GELU_CHAIN_TERM if DERIVED else 0.0)) * f['t'].abs() if gelu else chain
    du_bound = dy.abs() * (G2 * chain + GELU_GRAD_ERR) if gelu else torch.zeros_like(du)
    en = dict(y=_bound_entry(f['y'], y_bound, dtype), du=_bound_entry(du, du_bound, dtype))
    # the form that keeps no du: d = the du bound with the half ulp of du's own rounding to T
    d = du_bound + half_ulp(du, dtype)
    dx, A_dx = dx_ref(du, w, k)
    d_taps, _ = conv_ref(d, w.abs(), None, k, -1)
    fused = dict(dx=_bound_entry(dx, d_taps + n * U24 * A_dx + under, dtype))
    fused['dw'], fused['db'] = _sum_entries(x, to_storage(du, dtype), k, dtype, extra_d=d)
    return Yard(case=case, dtype=dtype, inp=inp, fwd=f, du=du, entries=en, fused=fused)


def judge(Y, got, only=None, form=None, rows=0):
    """{output: Verdict}.  got: any of y, du, dx, dw, db.  With du among them, dx / dw / db are held to what follows from the du that was
    written (the tight check); without it to the float64 du and the d term.  form / rows: the 3 x 3 form whose kernels produced `got`
    (None: no kernel, a CPU statement), for the DERIVED floor of dw / db below."""
    what = f'{Y.case["id"]} {Y.dtype}'
    en = dict(Y.entries)
    if got.get('du') is not None:
        k, w = Y.case['k'], Y.inp['w']
        du_got = got['du'].detach().cpu().double().reshape(Y.du.shape)
        dxp, Ap = dx_ref(du_got, w, k)
        en['dx'] = _bound_entry(dxp, k * k * (U24 * Ap + (UNDERFLOW if DERIVED else 0.0)), Y.dtype)
        en['dw'], en['db'] = _sum_entries(Y.inp['x'], du_got, k, Y.dtype)
    else:
        en.update(Y.fused)
    if DERIVED and form is not None and Y.case['cls'] == 'negative':
        # DERIVED floor of dw / db, class `negative` (b = -6): du = dy gelu'(t) with gelu' = -1e-8 ... -1e-4 over t = -6 +- 1.5, so a handful of
        # the pixels carry a column's sum (the largest term is 37 % of sum |terms| in the median column of (2, 9, 22, 640), against 4 % in
        # `plain`).  Every rounding after such a term has entered acts on the whole result instead of averaging out over the terms, and
        # FLOOR 4 -- the size of four roundings of the scale -- is not enough for ANY order of additions but a lucky one: the plain sequential
        # fp32 sum of the same terms in another order is at 20 and more (test_another_order_of_the_fp32_sum_needs_the_negative_floor, no kernel
        # involved).  The floor is the number of additions on the term's way through the form's reduction.
        fl = float(wgrad_roundings(form, Y.dtype, *Y.case['shape'], rows))
        en['dw'], en['db'] = dict(en['dw'], floor=fl), dict(en['db'], floor=fl)
    return R.judge(en, got, what, only)


# ---- statements that produce what a kernel call returns (for the CPU tests) -----------------------------------------------------------
def _store(t64, dtype):
    """float64 -> the storage type, rounded ONCE."""
    return X.round_bf16(t64) if dtype == BF else t64.to(F32)


def statement64(Y, mut=None):
    """The float64 statement with du rounded to the storage type in between (as every form does), every output rounded once; `mut`: one of
    MUTANTS.  -> dict(y, du, dx, dw, db)."""
    case, inp, dtype = Y.case, Y.inp, Y.dtype
    k, gelu, x, dy, w, b = case['k'], case['gelu'], inp['x'], inp['dy'], inp['w'], inp['b']
    f = fwd_ref(x, w, b, k, gelu, mut)
    du = _store(du_ref(f['t'], dy, gelu, b, mut), dtype)
    dx, _ = dx_ref(du.double(), w, k, mut)
    R_, _ = walk_plan(*case['shape'])
    dw, db, _, _ = wgrad_ref(x, du.double(), k, mut, seam_row=min(R_, case['shape'][1] - 1))
    if mut == 'db_over_dy':
        db = dy.sum((0, 1, 2))
    y = X.trunc_bf16(f['y'].float()) if mut == 'trunc_bf16' else _store(f['y'], dtype)
    return dict(y=y, du=du, dx=_store(dx, dtype), dw=dw.float(), db=db.float())


def statement32(Y):
    """The plain fp32 CPU statement: F.conv2d(groups = C) and F.gelu in fp32 with autograd; du is stored in the storage type between pass A
    and the passes that read it, as every form does.  -> dict(y, du, dx, dw, db)."""
    case, inp, dtype = Y.case, Y.inp, Y.dtype
    (B, H, W, C), k, gelu = case['shape'], case['k'], case['gelu']
    nchw = lambda t: t.float().permute(0, 3, 1, 2).contiguous()           # noqa: E731
    back = lambda t: t.permute(0, 2, 3, 1).contiguous()                    # noqa: E731
    xr = nchw(inp['x']).requires_grad_(True)
    wr = inp['w'].reshape(C, 1, k, k).clone().requires_grad_(True)
    br = torch.zeros(C) if inp['b'] is None else inp['b'].clone()
    br.requires_grad_(True)
    t = F.conv2d(xr, wr, br, padding=k // 2, groups=C)
    tl = t.detach().requires_grad_(True)
    y = F.gelu(tl) if gelu else tl * 1.0
    y.backward(nchw(inp['dy']))
    du = tl.grad.to(dtype)
    t.backward(du.float())
    return dict(y=back(y.detach()).to(dtype), du=back(du), dx=back(xr.grad).to(dtype), dw=wr.grad.reshape(C, k * k), db=br.grad)


# name -> (substrings that select the cases it is tried on, the outputs that may reject it, bf16 only)
MUTANTS = {
    'tap_dropped_last_col': (('dw3-plain-2x2x5x24-gelu', 'dw3-plain-2x9x22x640-id', 'dw7-plain-2x7x9x40'), ('y',), False),
    'seam_row_twice': (('dw3-plain-1x70x6x136-gelu', 'dw3-plain-2x130x7x16-id'), ('dw',), False),
    'bias_left_out_bwd': (('dw3-plain-2x9x22x640-gelu', 'dw3-negative-2x2x5x24-gelu'), ('du',), False),
    'kernel_not_flipped': (('dw3-plain-2x2x5x24-gelu', 'dw3-plain-2x9x22x640-id', 'dw7-plain-2x3x5x24'), ('dx',), False),
    'trunc_bf16': (('dw3-plain-2x9x22x640-gelu', 'dw3-plain-2x2x5x24-id', 'dw7-plain-2x7x9x40'), ('y',), True),
    'tanh_gelu': (('dw3-plain-2x9x22x640-gelu', 'dw3-plain-2x2x5x24-gelu'), ('y', 'du'), False),
    'db_over_dy': (('dw3-plain-2x9x22x640-gelu', 'dw3-sparse-2x2x5x24-gelu'), ('db',), False),
}

CASE_BY_ID = {c['id']: c for c in cases3() + cases7()}


# ---- the sampled reference of the one large 7 x 7 case ------------------------------------------------------------------------------
def lattice_i8(shape, g):
    """X.lattice as int8 (a 67 M-element map as float64 would be half a gigabyte)."""
    idx = torch.randint(0, 6, tuple(shape), generator=g, dtype=torch.int8)
    return idx - 3 + (idx >= 3).to(torch.int8)


def sample_pixels(B, H, W, count, g):
    """[(b, y, x)] as a [N][3] tensor: `count` random pixels, the four corners and one full border row and column of the first and last image."""
    pts = [torch.stack([torch.randint(0, n, (count,), generator=g) for n in (B, H, W)], 1)]
    for b in (0, B - 1):
        pts.append(torch.tensor([[b, yy, xx] for yy in (0, H - 1) for xx in (0, W - 1)]))
        pts.append(torch.tensor([[b, 0 if b == 0 else H - 1, xx] for xx in range(W)]))
        pts.append(torch.tensor([[b, yy, W - 1 if b == 0 else 0] for yy in range(H)]))
    return torch.cat(pts)


def gathered_conv7(t_i8, w64, bias64, pix, sign):
    """float64 b + sum_k w_k t[p + sign off_k] at the pixels `pix` only (all channels) of an int8 [B][H][W][C] map."""
    B, H, W, C = t_i8.shape
    out = torch.zeros(pix.shape[0], C, dtype=F64) if bias64 is None else bias64.double().expand(pix.shape[0], C).clone()
    flat = t_i8.reshape(-1, C)
    for i, (ky, kx) in enumerate(taps(7)):
        yy, xx = pix[:, 1] + sign * (ky - 3), pix[:, 2] + sign * (kx - 3)
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        rows = (pix[:, 0] * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1)
        out += flat[rows].double() * ok[:, None] * w64[:, i]
    return out
