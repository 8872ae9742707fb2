"""Float64 statements of the resize family of csrc/resize.hip and csrc/fuse_map.hip -- bilinear resize and its transpose, the fused
upsample-add (+ statistics), the folded head's stride-4 map (segf_fuse_map_248) and its transposed form, AdaptiveAvgPool2d and the nearest
resize -- their plain fp32 statements, the input classes, the case tables of tests/test_resize_float64.py and the mutants that the
comparison must reject.  Importable without a GPU.

Every operation is stated from include/segfac.h as DENSE 1-D float64 operators: a resize is  R_y (x) R_x  applied to the NHWC map, every
transposed resize is its transpose.  This is deliberately not the gather form of the kernels, and not F.interpolate (which only verifies
the references, tests/test_resize_float64.py::test_reference_*).  Activations enter already rounded to the storage type
(norm_refs.to_storage).  Each reference returns, beside the value, the per-element `scale`: the float64 sum of |weight x value| over
the element's terms, i.e. the same operators applied to |x|.

Comparator: norm_refs.compare, unchanged.  Elementwise outputs: class `elementwise`, group = one output pixel's channel row; column sums:
class `reduction` (scale = sum of |terms|; the sum of squares for the second row).  e_ref is the error against float64 of torch's fp32
F.interpolate / adaptive_avg_pool2d / autograd on the CPU (fused forms: those fp32 ops composed in the obvious order), never a kernel.

DERIVED (read where norm_refs.DERIVED is read): `coord_terms_*` and `stats_roundings` below.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import exact_inputs as X
import norm_refs as R

BF, F32, F64 = R.BF, R.F32, R.F64
U24 = R.U24
DT_ID = {F32: 'fp32', BF: 'bf16'}
CLASSES = ('plain', 'offset', 'sparse', 'const')


# ---- 1-D operators ----------------------------------------------------------------------------------------------------------------
def axis_coord(n_in, n_out, align_corners):
    """ATen's source coordinate of every destination index, in float64 -> (i0, i1, l, s)."""
    d = torch.arange(n_out, dtype=F64)
    if align_corners:
        s = d * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=F64)
    else:
        s = ((d + 0.5) * n_in / n_out - 0.5).clamp_min(0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0, s


def axis_matrix(n_in, n_out, align_corners):
    """R [n_out][n_in]: row d holds 1 - l at i0 and l at i1 (added where the two coincide)."""
    i0, i1, l, _ = axis_coord(n_in, n_out, align_corners)
    m = torch.zeros(n_out, n_in, dtype=F64)
    d = torch.arange(n_out)
    m.index_put_((d, i0), 1 - l, accumulate=True)
    m.index_put_((d, i1), l, accumulate=True)
    return m


def pool_matrix(n_in, S):
    """AdaptiveAvgPool bins [floor(i * in / S), ceil((i + 1) * in / S)): P [S][n_in]."""
    m = torch.zeros(S, n_in, dtype=F64)
    for i in range(S):
        a, b = (i * n_in) // S, -(-((i + 1) * n_in) // S)
        m[i, a:b] = 1.0 / (b - a)
    return m


def nearest_index(n_in, n_out):
    """Source index of every destination: integer ratios Y // (H // h); otherwise ATen's rule, which is SPECIFIED in fp32:
    min(int(floorf(Y * (float)h / H)), h - 1)."""
    d = np.arange(n_out)
    if n_out % n_in == 0:
        return torch.from_numpy(d // (n_out // n_in))
    scale = np.float32(n_in) / np.float32(n_out)
    return torch.from_numpy(np.minimum(np.floor(d.astype(np.float32) * scale).astype(np.int64), n_in - 1))


def nearest_matrix(n_in, n_out):
    m = torch.zeros(n_out, n_in, dtype=F64)
    m[torch.arange(n_out), nearest_index(n_in, n_out)] = 1.0
    return m


def up(My, Mx, x):
    """(My (x) Mx) x: x [B][h][w][C] -> [B][H][W][C]."""
    return torch.einsum('Yy,Xx,byxc->bYXc', My, Mx, x)


def down(My, Mx, d):
    """The transpose: d [B][H][W][C] -> [B][h][w][C]."""
    return torch.einsum('Yy,Xx,bYXc->byxc', My, Mx, d)


# ---- DERIVED: the coordinate term ------------------------------------------------------------------------------------------------
# For ratios other than 1, 2, 4, 8 (16: every power of two is exact) and for align_corners=True the fp32 source coordinate carries
# its own roundings, and hipcc may contract scale * (d + 0.5f) - 0.5f into one fma that ATen does not have: the kernel's l differs
# from torch's fp32 l, so e_ref cannot carry it.  s passes through three roundings (the quotient in / out, the product, the
# subtraction), each at most 2^-24 of a value no larger than s + 1:
#     |ds| <= COORD_ROUNDINGS * 2^-24 * (s + 1).
# out = (1 - l_y) [(1 - l_x) v00 + l_x v01] + l_y [(1 - l_x) v10 + l_x v11] is linear in each l, and l = s - i0 exactly, so to first order
#     |d out| <= ds_y |d out / d l_y| + ds_x |d out / d l_x|,   d out / d l_y = (1 - l_x)(v10 - v00) + l_x (v11 - v01)   (a blend of tap differences)
# Where s is an integer in float64 (l = 0: align_corners=True hits these) the rounded s may fall on either side of it, so the slope
# is the larger of the two one-sided ones (taps (i0 - 1, i0) and (i0, i0 + 1)); out is continuous there.
# Transposed resizes: din[y][x] = sum_YX w_y(Y, y) w_x(X, x) dy[Y][X]; every weight moves by at most ds, so
#     |d din| <= sum over the output pixels whose either candidate tap can be (y, x) of |dy| (ds_y |+-1| w_x + w_y ds_x |+-1|).
COORD_ROUNDINGS = 3.0


def coord_exact(n_in, n_out, align_corners):
    r = n_out // n_in
    return not align_corners and n_out % n_in == 0 and r & (r - 1) == 0


def axis_slopes(n_in, n_out, align_corners):
    """(ds [n_out], Dr, Dl [n_out][n_in]): the bound of the coordinate's error and the signed d(row of axis_matrix) / dl taken to
    the right (taps i0, i1) and to the left of an integer s (taps i0 - 1, i0; equal to Dr elsewhere)."""
    i0, i1, l, s = axis_coord(n_in, n_out, align_corners)
    ds = torch.zeros(n_out, dtype=F64) if coord_exact(n_in, n_out, align_corners) else COORD_ROUNDINGS * U24 * (s + 1)
    d = torch.arange(n_out)
    Dr = torch.zeros(n_out, n_in, dtype=F64)
    Dr.index_put_((d, i1), torch.ones(n_out, dtype=F64), accumulate=True)
    Dr.index_put_((d, i0), -torch.ones(n_out, dtype=F64), accumulate=True)
    Dl = Dr.clone()
    for k in torch.nonzero((l == 0) & (i0 > 0)).flatten().tolist():
        Dl[k] = 0
        Dl[k, i0[k]], Dl[k, i0[k] - 1] = 1.0, -1.0
    return ds, Dr, Dl


def coord_terms_fwd(x, H, W, ac):
    h, w = x.shape[1:3]
    Ry, Rx = axis_matrix(h, H, ac), axis_matrix(w, W, ac)
    dsy, Dyr, Dyl = axis_slopes(h, H, ac)
    dsx, Dxr, Dxl = axis_slopes(w, W, ac)
    ey = torch.maximum(up(Dyr, Rx, x).abs(), up(Dyl, Rx, x).abs()) * dsy[None, :, None, None]
    ex = torch.maximum(up(Ry, Dxr, x).abs(), up(Ry, Dxl, x).abs()) * dsx[None, None, :, None]
    return ey + ex


def coord_terms_bwd(dy, h, w, ac):
    H, W = dy.shape[1:3]
    Ry, Rx = axis_matrix(h, H, ac), axis_matrix(w, W, ac)
    dsy, Dyr, Dyl = axis_slopes(h, H, ac)
    dsx, Dxr, Dxl = axis_slopes(w, W, ac)
    Ay = torch.maximum(Dyr.abs(), Dyl.abs()) * dsy[:, None]
    Ax = torch.maximum(Dxr.abs(), Dxl.abs()) * dsx[:, None]
    return down(Ay, Rx, dy.abs()) + down(Ry, Ax, dy.abs())


# ---- references: -> (value, scale) ------------------------------------------------------------------------------------------------
def bilinear_fwd_ref(x, H, W, ac=False):
    Ry, Rx = axis_matrix(x.shape[1], H, ac), axis_matrix(x.shape[2], W, ac)
    return up(Ry, Rx, x), up(Ry, Rx, x.abs())


def bilinear_bwd_ref(dy, h, w, ac=False):
    Ry, Rx = axis_matrix(h, dy.shape[1], ac), axis_matrix(w, dy.shape[2], ac)
    return down(Ry, Rx, dy), down(Ry, Rx, dy.abs())


def to_nchw_ref(x, H, W):
    v, s = bilinear_fwd_ref(x, H, W, False)
    return v.permute(0, 3, 1, 2), s.permute(0, 3, 1, 2)


def upsample_add_ref(base, srcs, ac=False):
    v, s = base.clone(), base.abs()
    for t in srcs:
        a, b = bilinear_fwd_ref(t, base.shape[1], base.shape[2], ac)
        v, s = v + a, s + b
    return v, s


def channel_sums_ref(t):
    """sums [2][C] = per-channel (sum, sum of squares) over every pixel of t [B][H][W][C], and their scales (sum of |terms|; the sum of
    squares itself).  segf_upsample_add_stats: t = the STORED, rounded output; segf_fuse_map_248: t = the result BEFORE the bf16 store."""
    f = t.reshape(-1, t.shape[-1])
    return torch.stack([f.sum(0), (f * f).sum(0)]), torch.stack([f.abs().sum(0), (f * f).sum(0)])


def fuse_map_ref(x1, g1, ts):
    """out = x1 G1^T + the three resizes; x1 [B][H][W][C1], g1 [C][C1], ts = the 1/2, 1/4, 1/8 maps."""
    v0, s0 = x1 @ g1.t(), x1.abs() @ g1.abs().t()
    v, s = upsample_add_ref(v0, ts, False)
    return v, s - v0.abs() + s0


def bilinear_bwd_248_ref(dy):
    H, W = dy.shape[1:3]
    return [bilinear_bwd_ref(dy, H // r, W // r, False) for r in (2, 4, 8)]


def adaptive_avgpool_ref(x, S, bwd=False, HW=None):
    """bwd=False: x [B][H][W][C] -> [B][S][S][C]; bwd=True: x = dout [B][S][S][C] -> din [B][H][W][C], HW = (H, W)."""
    H, W = HW if bwd else x.shape[1:3]
    Py, Px = pool_matrix(H, S), pool_matrix(W, S)
    return (down(Py, Px, x), down(Py, Px, x.abs())) if bwd else (up(Py, Px, x), up(Py, Px, x.abs()))


def nearest_up_ref(x, h, w, H, W, base=None, bwd=False):
    Ny, Nx = nearest_matrix(h, H), nearest_matrix(w, W)
    if bwd:
        return down(Ny, Nx, x), down(Ny, Nx, x.abs())
    v, s = up(Ny, Nx, x), up(Ny, Nx, x.abs())
    return (v, s) if base is None else (v + base, s + base.abs())


# ---- the plain fp32 statements: torch on the CPU ------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def interp32(x32, H, W, ac=False):
    return _nhwc(F.interpolate(_nchw(x32), size=(H, W), mode='bilinear', align_corners=ac))


def interp_bwd32(dy32, h, w, ac=False):
    B, H, W, C = dy32.shape
    x = torch.zeros(B, C, h, w, dtype=dy32.dtype, requires_grad=True)
    F.interpolate(x, size=(H, W), mode='bilinear', align_corners=ac).backward(_nchw(dy32))
    return _nhwc(x.grad)


def upsample_add32(base32, srcs32, ac=False):
    v = base32
    for t in srcs32:
        v = v + interp32(t, base32.shape[1], base32.shape[2], ac)
    return v


def pool32(x32, S, bwd=False, HW=None):
    if not bwd:
        return _nhwc(F.adaptive_avg_pool2d(_nchw(x32), S))
    B, _, _, C = x32.shape
    x = torch.zeros(B, C, *HW, dtype=x32.dtype, requires_grad=True)
    F.adaptive_avg_pool2d(x, S).backward(_nchw(x32))
    return _nhwc(x.grad)


def nearest32(x32, h, w, H, W, base32=None, bwd=False):
    if not bwd:
        v = _nhwc(F.interpolate(_nchw(x32), size=(H, W), mode='nearest'))
        return v if base32 is None else v + base32
    B, _, _, C = x32.shape
    x = torch.zeros(B, C, h, w, dtype=x32.dtype, requires_grad=True)
    F.interpolate(x, size=(H, W), mode='nearest').backward(_nchw(x32))
    return _nhwc(x.grad)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def make_map(cls, shape, g):
    """plain: randn.  offset: mean 100, sigma 1 (weights that do not sum to one, or a lost clamp share, show at 1e-2 of the result).
    sparse: 80 % exact zeros, the last image all zero when there is more than one.  const: one value k / 4 per channel.
    lattice: exact_inputs.lattice (float64, exact in bf16)."""
    if cls == 'lattice':
        return X.lattice(shape, g)
    z = torch.randn(tuple(shape), generator=g, dtype=F32)
    if cls == 'plain':
        return z
    if cls == 'offset':
        return z + 100
    if cls == 'sparse':
        z = z * (torch.rand(tuple(shape), generator=g) < 0.2)
        if shape[0] > 1:
            z[-1] = 0
        return z
    if cls == 'const':
        return R._dyadic(shape[-1], g).expand(tuple(shape)).clone()
    raise KeyError(cls)


def _in(cls, shape, g, dtype):
    t = make_map(cls, shape, g)
    return t if cls == 'lattice' else R.to_storage(t, dtype)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
def _fmt(v):
    if isinstance(v, tuple):
        return ('_' if v and isinstance(v[0], tuple) else 'x').join(_fmt(e) for e in v) or 'none'
    return str(v)


def _case(op, **kw):
    kw['op'] = op
    kw['id'] = op + '-' + '-'.join(f'{k}{_fmt(v)}' for k, v in kw.items() if k not in ('op', 'why'))
    return kw


# (B, (h, w), (H, W), C, align_corners): bilinear_fwd_kernel / bilinear_bwd_kernel / bilinear_to_nchw_kernel (ac = 0 rows)
RESIZE_CASES = [_case('resize', B=B, src=s, dst=d, C=C, ac=ac, why=why) for B, s, d, C, acs, why in (
    (2, (1, 1), (7, 9), 16, (0, 1), 'the in == 1 branch of out_range'),
    (2, (3, 7), (12, 9), 150, (0,), 'ragged last chunk, up and down scaling mixed'),
    (1, (13, 11), (37, 29), 24, (0, 1), 'a general ratio up'),
    (1, (37, 29), (13, 11), 8, (0, 1), 'down by more than 2: inputs without gradient are exact zeros'),
    (1, (5, 7), (5, 7), 8, (0,), 'identity'),
    (1, (6, 6), (1, 9), 8, (1,), 'out == 1'),
    (1, (4, 4), (8, 16), 8, (0,), 'integer but unequal ratios: not the fast path'),
    (1, (2, 2), (32, 32), 8, (0,), 'R = 16: not the fast path'),
) for ac in acs]
NCHW19_CASE = _case('resize', B=1, src=(3, 5), dst=(7, 9), C=19, ac=0, why='to_nchw with ldi > C')
# bilinear_bwd_int_kernel<T, R>: channel groups G = 1, 4, 8
INT_CASES = [_case('int', B=2, R=r, src=s, C=C) for r in (2, 4, 8) for s in ((5, 7), (1, 6), (6, 1)) for C in (24, 32, 64)]
# bilinear_bwd_248: (H / 8, W / 8); B alternates so that 1 and 2 both appear in every column of the table
MAPS_248 = ((1, 1), (1, 2), (2, 1), (3, 3), (1, 5), (5, 1), (4, 5))
BWD248_FORMS = (('valu', F32, 8), ('valu', F32, 32), ('valu', F32, 64), ('valu', BF, 40), ('valu-forced', BF, 128), ('mfma', BF, 128), ('mfma', BF, 256))
BWD248_CASES = [_case('bwd248', B=1 + (i + j) % 2, m8=m, C=C, form=form, dt=DT_ID[dt])
                for j, (form, dt, C) in enumerate(BWD248_FORMS) for i, m in enumerate(MAPS_248)]
PYRAMID = lambda H, W: ((H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8))        # noqa: E731
_GEN = ((4, 3), (2, 5), (5, 4))
UPADD_CASES = (
    [_case('upadd', B=2, dst=(9, 7), C=16, srcs=_GEN[:n], ac=0, form='generic') for n in range(4)]
    + [_case('upadd', B=2, dst=(9, 7), C=16, srcs=_GEN, ac=1, form='generic'),
       _case('upadd', B=1, dst=(12, 20), C=8, srcs=((6, 10), (3, 5), (2, 3)), ac=0, form='generic'),
       _case('upadd', B=2, dst=(16, 24), C=40, srcs=PYRAMID(16, 24), ac=0, form='generic-forced')]
    + [_case('upadd', B=B, dst=d, C=C, srcs=PYRAMID(*d), ac=0, form='248') for B, d, C in ((1, (8, 8), 8), (2, (16, 24), 40), (1, (8, 40), 104))])
STATS_CASES = [_case('upadd', B=B, dst=d, C=C, srcs=PYRAMID(*d), ac=0, form='stats') for B, d, C in ((2, (16, 24), 8), (2, (16, 24), 104), (1, (8, 16), 2048))]
# fuse_map_kernel<KS1, STATS>: (C1, C, B, (H, W)); ld: row strides above the widths
FUSE_CASES = [_case('fuse', k1=C1, C=C, B=B, dst=d, ld=ld) for C1, C, B, d, ld in (
    (32, 128, 1, (8, 8), 0), (64, 128, 1, (8, 24), 0), (32, 768, 1, (24, 8), 0), (64, 768, 2, (24, 24), 0), (32, 128, 2, (24, 24), 1),
    (64, 768, 2, (64, 64), 0))]
POOL_CASES = [_case('pool', B=2, S=S, src=m) for S in (1, 2, 3, 6) for m in ((7, 5), (6, 6), (1, 1), (2, 3))]
NEAREST_CASES = [_case('nearest', B=2, src=(h, w), dst=(H, W))
                 for h, w, H, W in ((3, 3, 5, 6), (10, 12, 9, 12), (5, 6, 10, 12), (4, 7, 12, 21), (7, 5, 16, 9), (1, 1, 3, 4), (6, 9, 4, 5))]
POOL_C = NEAREST_C = (8, 24)
BIG = 2_000_000           # above this many output elements a case runs `plain` (and `lattice`) only


def case_classes(case, C=None):
    d = case.get('dst') or case.get('src') or tuple(8 * v for v in case['m8'])
    n = case['B'] * d[0] * d[1] * (C or case.get('C', 24))
    return ('plain',) if n > BIG else CLASSES


def is_exact_case(case):
    """Lattice inputs make every product and sum exact in fp32: weights (a / 16)(b / 16) (a / 32 at ratio 16), at most 256 terms."""
    op = case['op']
    if op == 'resize':
        return all(coord_exact(s, d, case['ac']) for s, d in zip(case['src'], case['dst']))
    if op == 'upadd':
        return all(coord_exact(s, d, case['ac']) for t in case['srcs'] for s, d in zip(t, case['dst']))
    return op in ('int', 'bwd248', 'fuse')


# ---- yards: inputs, float64 results, e_ref and scale of every output of a case ----------------------------------------------------------
def _elem(ref, st32, scale, store, extra=None, dim=-1):
    en = R._entry(ref, R.group_err(st32, ref, dim), scale, store)
    if extra is not None and R.DERIVED:
        en['extra'] = extra
    return en


def _sums(terms64, terms32):
    ref, scale = channel_sums_ref(terms64)
    f = terms32.reshape(-1, terms32.shape[-1])
    e = torch.stack([R.sums_err(f, ref[0]), R.sums_err(f * f, ref[1])])
    return R._entry(ref, e, scale, F32, 'reduction')


# DERIVED floor of the sums of segf_upsample_add_stats.  The issue's floor of 4 is the size of a few roundings of the whole sum; the
# sum of squares (every term >= 0, so no rounding is made on a partial sum that cancellation kept small) passes through many more on its
# way through upsample_add_248_kernel<T, true> and colreduce_finalize_kernel, each at most 2^-24 of a partial sum <= sum |terms|:
#   a thread adds the 4 pixels of each of its strips, one after the other           4 * strips per thread
#   the first thread of a chunk adds the later threads of the workgroup in order    ceil(256 / (C / 8)) - 1
#   the finalize adds every 16th workgroup partial, then its 16 slices              ceil(blocks / 16) + 16
# The plain fp32 sum taken in this order on the CPU is outside max(2 e_ref, 4 * 2^-24 * scale) with no kernel involved
# (tests/test_resize_float64.py::test_stats_order_of_the_fp32_sum_needs_the_derived_floor).
def stats_plan(B, H, W, C):
    """(workgroups, strips between two strips of one thread) of upsample_add_248_kernel<T, true>: colfixed_blocks of csrc/common.h
    restated (two strips per thread, at most 16384 workgroups, a multiple of what keeps every thread on one chunk)."""
    nch, units = C // 8, B * H * (W // 4)
    unit = nch // math.gcd(nch, 256)
    want = max(1, min(-(-(-(-units // 2) * nch) // 256), 16384))
    blocks = -(-want // unit) * unit
    return blocks, blocks * 256 // nch


def stats_roundings(B, H, W, C):
    blocks, ustep = stats_plan(B, H, W, C)
    return 4 * -(-(B * H * (W // 4)) // ustep) + (-(-256 // (C // 8)) - 1) + -(-blocks // 16) + 16


def stats_order_sums32(t32):
    """sums [2][C] of t32 [B][H][W][C] in plain fp32 (numpy), added in the order of upsample_add_248_kernel<T, true> + the finalize."""
    B, H, W, C = t32.shape
    nch = C // 8
    blocks, ustep = stats_plan(B, H, W, C)
    u = t32.float().reshape(-1, 4, C).numpy()
    out = []
    for f in (lambda a: a, lambda a: a * a):
        z = np.zeros(C, np.float32)
        parts = []
        for j in range(min(ustep, u.shape[0])):             # thread j of every chunk: strips j, j + ustep, ...
            acc = z
            for k in range(j, u.shape[0], ustep):
                for p in range(4):
                    acc = acc + f(u[k, p])
            parts.append(acc)
        per = max(256 // nch, 1)                                # threads of one chunk in a workgroup
        slices = [z] * 16
        for b in range(blocks):
            a = z
            for q in parts[b * per:(b + 1) * per]:
                a = a + q
            slices[b % 16] = slices[b % 16] + a
        tot = z
        for q in slices:
            tot = tot + q
        out.append(torch.from_numpy(tot))
    return torch.stack(out)


def sums_entry_of_stored(out, shape):
    """The `sums` entry of segf_upsample_add_stats for a STORED output (any device, fp32 or bf16) of geometry shape = (B, H, W, C)."""
    t = out.detach().cpu()
    en = _sums(t.double(), t.float())
    if R.DERIVED:
        en['floor'] = float(stats_roundings(*shape))
    return en


@functools.lru_cache(maxsize=8)
def yard(case_id, dtype, cls, C=None):
    """-> Yard(case, dtype, cls, inp, entries, st): st = the fp32 statement's outputs, unrounded.  `lattice`: entries hold `ref` only."""
    case = CASE_BY_ID[case_id]
    g = X.gen(R.seed_of(f'{case_id}-{cls}-{C}'))
    op, B = case['op'], case['B']
    C = C or case['C']
    mk = lambda *hw_c: _in(cls, (B,) + hw_c, g, dtype)                 # noqa: E731
    f = lambda t: t.float()                                            # noqa: E731
    en, st = {}, {}
    if op in ('resize', 'int'):
        (h, w) = case['src']
        (H, W) = case['dst'] if op == 'resize' else (case['R'] * h, case['R'] * w)
        ac = bool(case.get('ac', 0))
        inp = dict(x=mk(h, w, C), dy=mk(H, W, C))
        st = dict(out=interp32(f(inp['x']), H, W, ac), din=interp_bwd32(f(inp['dy']), h, w, ac))
        v, s = bilinear_fwd_ref(inp['x'], H, W, ac)
        en['out'] = _elem(v, st['out'], s, dtype, coord_terms_fwd(inp['x'], H, W, ac))
        v, s = bilinear_bwd_ref(inp['dy'], h, w, ac)
        en['din'] = _elem(v, st['din'], s, dtype, coord_terms_bwd(inp['dy'], h, w, ac))
        if not ac:
            st['nchw'] = _nchw(st['out'])
            en['nchw'] = _elem(_nchw(en['out']['ref']), st['nchw'], _nchw(en['out']['scale']), F32,
                               _nchw(coord_terms_fwd(inp['x'], H, W, ac)), dim=1)
    elif op == 'bwd248':
        H, W = 8 * case['m8'][0], 8 * case['m8'][1]
        inp = dict(dy=mk(H, W, C))
        for r, (v, s) in zip((2, 4, 8), bilinear_bwd_248_ref(inp['dy'])):
            st[f'd{r}'] = interp_bwd32(f(inp['dy']), H // r, W // r)
            en[f'd{r}'] = _elem(v, st[f'd{r}'], s, dtype)
    elif op == 'upadd':
        H, W = case['dst']
        ac = bool(case['ac'])
        inp = dict(base=mk(H, W, C), srcs=[mk(h, w, C) for h, w in case['srcs']])
        st = dict(out=upsample_add32(f(inp['base']), [f(t) for t in inp['srcs']], ac))
        v, s = upsample_add_ref(inp['base'], inp['srcs'], ac)
        extra = sum((coord_terms_fwd(t, H, W, ac) for t in inp['srcs']), torch.zeros_like(v))
        en['out'] = _elem(v, st['out'], s, dtype, extra)
    elif op == 'fuse':
        H, W = case['dst']
        C1 = case['k1']
        gm = X.lattice((C, C1), g) if cls == 'lattice' else R.to_storage(0.3 * torch.randn(C, C1, generator=g), BF)
        inp = dict(x1=_in(cls, (B, H, W, C1), g, BF), g1=gm, ts=[_in(cls, (B, h, w, C), g, BF) for h, w in PYRAMID(H, W)])
        st = dict(out=upsample_add32(f(inp['x1']) @ f(gm).t(), [f(t) for t in inp['ts']]))
        v, s = fuse_map_ref(inp['x1'], gm, inp['ts'])
        en['out'] = _elem(v, st['out'], s, BF)
        en['sums'] = _sums(v, st['out'])
    elif op == 'pool':
        H, W = case['src']
        S = case['S']
        inp = dict(x=mk(H, W, C), dy=mk(S, S, C))
        st = dict(out=pool32(f(inp['x']), S), din=pool32(f(inp['dy']), S, True, (H, W)))
        v, s = adaptive_avgpool_ref(inp['x'], S)
        en['out'] = _elem(v, st['out'], s, dtype)
        v, s = adaptive_avgpool_ref(inp['dy'], S, True, (H, W))
        en['din'] = _elem(v, st['din'], s, dtype)
    elif op == 'nearest':
        (h, w), (H, W) = case['src'], case['dst']
        inp = dict(x=mk(h, w, C), base=mk(H, W, C), dy=mk(H, W, C))
        st = dict(out=nearest32(f(inp['x']), h, w, H, W), sum=nearest32(f(inp['x']), h, w, H, W, f(inp['base'])),
                  din=nearest32(f(inp['dy']), h, w, H, W, bwd=True))
        for name, (v, s) in (('out', nearest_up_ref(inp['x'], h, w, H, W)), ('sum', nearest_up_ref(inp['x'], h, w, H, W, inp['base'])),
                             ('din', nearest_up_ref(inp['dy'], h, w, H, W, bwd=True))):
            en[name] = _elem(v, st[name], s, dtype)
    else:
        raise KeyError(op)
    return R.Yard(case=case, dtype=dtype, cls=cls, inp=inp, entries=en, st=st)


ALL_CASES = RESIZE_CASES + [NCHW19_CASE] + INT_CASES + BWD248_CASES + UPADD_CASES + STATS_CASES + FUSE_CASES + POOL_CASES + NEAREST_CASES
CASE_BY_ID = {c['id']: c for c in ALL_CASES}


def case_dtypes(case):
    if case['op'] == 'fuse':
        return (BF,)
    if case['op'] == 'bwd248':
        return (F32,) if case['dt'] == 'fp32' else (BF,)
    return (F32, BF)


def case_channels(case):
    return POOL_C if case['op'] == 'pool' else NEAREST_C if case['op'] == 'nearest' else (None,)


def judge(Y, got, only=None):
    return R.judge(Y.entries, got, f'{Y.case["id"]} {Y.cls} {DT_ID[Y.dtype]}', only)


def stored(st, Y):
    """The fp32 statement's outputs as a kernel would leave them: rounded to each entry's storage type."""
    return {k: v.to(Y.entries[k]['store']) for k, v in st.items() if k in Y.entries}


# ---- mutants: wrong statements in fp32 on the CPU, as dense fp32 operators ---------------------------------------------------------------
def _f32m(m):
    return m.float()


def mutant_upsample_add(inp, name):
    """The 2-4-8 upsample-add in fp32 with one wrong tap.
    corner_dropped   the (y1, x1) tap of the 1/8 level is dropped on the first source row (y0 == 0): weights down to 1 / 256
    clamp_omitted    the index clamp is omitted at the right border: the edge source loses the share of the virtual source beyond it
    strip_swapped    x4 level: the strip's first pixel takes 0.375 / 0.625 the other way round
    None             the unmutated statement"""
    base = inp['base'].float()
    H, W = base.shape[1:3]
    v = base
    for lvl, t in enumerate(inp['srcs']):
        h, w = t.shape[1:3]
        Ry, Rx = axis_matrix(h, H, False), axis_matrix(w, W, False)
        if name == 'clamp_omitted' and lvl == 0:
            i0, i1, l, _ = axis_coord(w, W, False)
            for X_ in torch.nonzero(i0 == w - 1).flatten().tolist():
                Rx[X_, w - 1] = 1 - l[X_]
        if name == 'strip_swapped' and lvl == 1:
            i0, i1, l, _ = axis_coord(w, W, False)
            for X_ in range(4, W, 4):
                Rx[X_, i0[X_]], Rx[X_, i1[X_]] = l[X_].item(), 1 - l[X_].item()
        u = up(_f32m(Ry), _f32m(Rx), t.float())
        if name == 'corner_dropped' and lvl == 2:
            (y0, y1, ly, _), (x0, x1, lx, _) = axis_coord(h, H, False), axis_coord(w, W, False)
            Ly, Lx = torch.zeros(H, h, dtype=F64), torch.zeros(W, w, dtype=F64)
            rows = torch.nonzero((y0 == 0) & (y1 != y0)).flatten()
            Ly[rows, y1[rows]] = ly[rows]
            cols = torch.nonzero(x1 != x0).flatten()
            Lx[cols, x1[cols]] = lx[cols]
            u = u - up(_f32m(Ly), _f32m(Lx), t.float())
        v = v + u
    return v


def mutant_bwd(dy, h, w, name):
    """A transposed resize in fp32.
    row_twice    the second row of every input pixel's window is counted twice
    unwritten    an input pixel that no output touches keeps what the buffer held (1e-30) instead of 0"""
    H, W = dy.shape[1:3]
    Ry, Rx = axis_matrix(h, H, False), axis_matrix(w, W, False)
    if name == 'row_twice':
        for y in range(h):
            rows = torch.nonzero(Ry[:, y]).flatten()
            if rows.numel() > 1:
                Ry[rows[1], y] *= 2
    v = down(_f32m(Ry), _f32m(Rx), dy.float())
    if name == 'unwritten':
        touched = (Ry.abs().sum(0) > 0)[:, None] & (Rx.abs().sum(0) > 0)[None, :]
        assert not touched.all(), 'every input pixel has a gradient: not a case for this mutant'
        v = torch.where(touched[None, :, :, None], v, torch.full_like(v, 1e-30))
    return v
