"""Inputs whose right answer is EXACT and independent of summation order, their float64 / closed-form references, the comparison the
exact tests use, and mutants of the references (tests/test_exact_kernels.py).

Integer lattice: every operand element is drawn from {-3,-2,-1,1,2,3} (no zeros: every term matters to every output), optionally times a
power of two per tensor.  Such values are exact in bf16, every product is an integer of magnitude <= 9 and every partial sum over K terms
is an integer below 9 K, exact in fp32 while 9 K < 2^24.  So an fp32 result must equal the float64 result bit for bit and a bf16 result
must equal it rounded ONCE to nearest even, whatever the tile shape, K slicing or MFMA form.

Known-answer attention: `selector` (every query picks exactly one key: the softmax is exactly one-hot in fp32) and `uniform` (Q = 0:
every probability is exactly 1 / Nkv).
"""
import math

import torch
import torch.nn.functional as F

LATTICE = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)
FP32_EXACT_TERMS = (1 << 24) // 9          # a lattice dot product of fewer terms is exact in fp32 in any order


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice(shape, g, pow2=0):
    """float64 tensor of lattice values times 2^pow2."""
    idx = torch.randint(0, 6, tuple(shape), generator=g, dtype=torch.int8)
    return (idx - 3 + (idx >= 3)).double() * (2.0 ** pow2)               # 0..5 -> -3, -2, -1, 1, 2, 3


def integers(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def pow2s(shape, g, exps=(-2, -1, 0, 1)):
    idx = torch.randint(0, len(exps), tuple(shape), generator=g)
    return torch.tensor([2.0 ** e for e in exps], dtype=torch.float64)[idx]


# ---- rounding and the comparison ------------------------------------------------------------------------------------------------
def round_bf16(x64):
    """float64 -> the nearest bf16 (ties to even), rounded ONCE from the float64 value (no fp32 step in between).  Returned as bf16."""
    x64 = x64.contiguous()
    bits = x64.view(torch.int64)
    drop = 52 - 7                                        # bf16 keeps 7 mantissa bits
    lsb = (bits >> drop) & 1
    r = ((bits + ((1 << (drop - 1)) - 1) + lsb) >> drop) << drop
    return r.view(torch.float64).to(torch.bfloat16)      # exactly representable now: the cast cannot round again


def trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (the WRONG store: a mutant)."""
    return (x32.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def expected(ref64, dtype):
    """The one right answer in the output type."""
    if dtype == torch.bfloat16:
        return round_bf16(ref64)
    r = ref64.to(dtype)
    assert dtype != torch.float32 or torch.equal(r.double(), ref64), 'the reference is not exact in fp32: not a lattice problem'
    return r


def _raw(t):
    """Raw words of a tensor with -0 mapped to +0 (the sign of an exact zero is the only thing the derivation leaves open)."""
    t = t.detach().cpu().contiguous()
    w = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64)
    return torch.where(t == 0, torch.zeros_like(w), w)


def mismatch_report(got, want, what='', ulp=0):
    """None when `got` equals `want` bit for bit (both in the output type, same shape), else a description of the wrong elements: their
    count, the first few (index, got, expected) and whether they share a row, a column or a residue modulo 16 / 32 / 128 / 256 -- with
    exact inputs the pattern names the tile or lane at fault.  ulp = 1 allows one unit in the last place (adjacent raw words)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f'{what}: got {got.dtype} {tuple(got.shape)}, expected {want.dtype} {tuple(want.shape)}'
    a, b = _raw(got), _raw(want)
    if ulp == 0:
        if torch.equal(a, b):
            return None
        bad = a != b
    else:
        # adjacent words of one sign are adjacent values; finite values only
        d = (a.to(torch.int64) - b.to(torch.int64)).abs()
        bad = (d > ulp) | ~torch.isfinite(got.float())
        if not bad.any():
            return None
    g2 = got.reshape(-1, got.shape[-1]) if got.dim() > 1 else got.reshape(1, -1)
    w2 = want.reshape(g2.shape)
    bad2 = bad.reshape(g2.shape)
    idx = bad2.nonzero()
    n = idx.shape[0]
    lines = [f'{what}: {n} of {bad2.numel()} elements wrong ({100.0 * n / bad2.numel():.3g} %), shape {tuple(got.shape)} '
             f'viewed as {tuple(g2.shape)}']
    for r, c in idx[:6].tolist():
        lines.append(f'  (row {r}, col {c}): got {g2[r, c].item()!r}, expected {w2[r, c].item()!r}')
    rows, cols = idx[:, 0], idx[:, 1]
    for name, v in (('row', rows), ('column', cols)):
        u = torch.unique(v)
        if u.numel() == 1:
            lines.append(f'  all in {name} {u.item()}')
        else:
            lines.append(f'  {name}s {u.min().item()} .. {u.max().item()} ({u.numel()} distinct)')
        for m in (16, 32, 128, 256):
            res = torch.unique(v % m)
            if res.numel() <= m // 4 and u.numel() > res.numel():
                lines.append(f'  {name} mod {m} in {res.tolist()[:16]}')
    err = (g2.double() - w2.double()).abs()[bad2]
    lines.append(f'  largest |got - expected| {err.max().item():.6g}, smallest {err.min().item():.6g}')
    return '\n'.join(lines)


def assert_exact(got, ref64, what='', ulp=0):
    """`got` (fp32 or bf16, any device) against the float64 reference: equal to it (fp32) / to it rounded once to nearest even (bf16)."""
    msg = mismatch_report(got, expected(ref64.reshape(got.shape), got.dtype), what, ulp)
    assert msg is None, msg


def is_exact(got, ref64, ulp=0):
    return mismatch_report(got, expected(ref64.reshape(got.shape), got.dtype), '', ulp) is None


# ---- linear algebra ---------------------------------------------------------------------------------------------------------------
def matmul64(a, b):
    """a @ b in float64.  Products above 8 GFLOP run torch's float64 matmul on the GPU when there is one (the vendor BLAS: none of this
    project's code; integer lattice sums are exact in float64 in any order, so where it runs cannot change the reference)."""
    a, b = a.double(), b.double()
    if 2.0 * a.shape[0] * a.shape[1] * b.shape[1] > 8e9 and torch.cuda.is_available():
        return (a.cuda() @ b.cuda()).cpu()
    return a @ b


def gemm_operand_shapes(layout, M, N, K):
    return {0: ((M, K), (N, K)), 1: ((M, K), (K, N)), 2: ((K, M), (K, N))}[layout]


def gemm_ref(layout, A, B, bias=None, residual=None, rscale=None, rows_per_group=1):
    """include/segfac.h segf_gemm in float64: v = sum_k A(m,k) B(k,n) (+ bias[n]); v = residual + rscale[m / rows_per_group] * v."""
    A, B = A.double(), B.double()
    v = matmul64(A, B.t()) if layout == 0 else matmul64(A, B) if layout == 1 else matmul64(A.t(), B)
    if bias is not None:
        v = v + bias.double()[None, :]
    if residual is not None:
        if rscale is not None:
            m = torch.arange(v.shape[0]) // rows_per_group
            v = v * rscale.double()[m][:, None]
        v = residual.double() + v
    return v


def gemm_pro_ref(layout, A, B, scale, shift, rows_per_group, act, bias=None):
    """segf_gemm_pro in float64: the activation operand is act(x * scale[g] + shift[g]) rounded to bf16 (exact on these inputs)."""
    X = (A if layout == 0 else B).double()
    g = torch.arange(X.shape[0]) // rows_per_group
    X = X * scale.double()[g] + shift.double()[g]
    if act == 1:
        X = X.clamp(min=0)
    elif act == 2:
        X = X.clamp(min=0, max=6)
    assert torch.equal(X.to(torch.bfloat16).double(), X), 'the normalised operand must be exact in bf16'
    return gemm_ref(layout, X, B, bias) if layout == 0 else gemm_ref(layout, A, X, bias)


def dw_db_ref(dy, x):
    """segf_gemm_dw_db: (dy^T x, column sums of dy), dy [K][M], x [K][N]."""
    return matmul64(dy.t(), x), dy.double().sum(0)


def _nchw(t, B, H, W):
    return t.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _tok(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv3x3_ref(mode, x, w, B, H, W, Cin, Cout, bias=None):
    """segf_conv3x3 in float64 (NHWC rows, stride 1, pad 1).  mode 0: x [P][Cin], w [Cout][9 Cin] ((ky,kx) major, ci minor) -> [P][Cout];
    mode 1: x := dy [P][Cout], w := wt [Cin][9 Cout] ([ci][(ky,kx)][co]) -> dx [P][Cin]; mode 2: x [P][Cin], w := dy [P][Cout] ->
    dw [Cout][9 Cin]."""
    P = B * H * W
    xp = F.pad(x.double().reshape(B, H, W, -1), (0, 0, 1, 1, 1, 1))                      # [B][H+2][W+2][C]
    sh = lambda ky, kx: xp[:, ky:ky + H, kx:kx + W].reshape(P, -1)                       # noqa: E731   x[pix + off(ky, kx)]
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    if mode == 0:
        w3 = w.double().reshape(Cout, 9, Cin)
        y = sum(matmul64(sh(ky, kx), w3[:, t].t()) for t, (ky, kx) in enumerate(taps))
        return y if bias is None else y + bias.double()[None]
    if mode == 1:
        # dx[pix][ci] = sum_{tap, co} dy[pix - off(tap)][co] wt[ci][tap][co]: the shifted read of dy uses the mirrored tap
        w3 = w.double().reshape(Cin, 9, Cout)
        return sum(matmul64(sh(2 - ky, 2 - kx), w3[:, t].t()) for t, (ky, kx) in enumerate(taps))
    dy = w.double()
    return torch.stack([matmul64(dy.t(), sh(ky, kx)) for ky, kx in taps], 1).reshape(Cout, 9 * Cin)


def dwconv_ref(x, w, bias, B, H, W, C, k):
    """Depthwise k x k conv + bias on NHWC rows, stride 1, pad k // 2; w [C][k*k]."""
    w4 = w.double().reshape(C, 1, k, k)
    return _tok(F.conv2d(_nchw(x, B, H, W), w4, None if bias is None else bias.double(), padding=k // 2, groups=C))


def dwconv_bwd_ref(x, w, dy, B, H, W, C, k):
    """(dx, dw [C][k*k], db [C]) of dwconv_ref."""
    xn = _nchw(x, B, H, W).requires_grad_(True)
    w4 = w.double().reshape(C, 1, k, k).requires_grad_(True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(xn, w4, b, padding=k // 2, groups=C).backward(_nchw(dy, B, H, W))
    return _tok(xn.grad), w4.grad.reshape(C, k * k), b.grad


def bilinear_ref(x, B, h, w, C, H, W):
    """F.interpolate(bilinear, align_corners=False) on NHWC rows; by 2, 4, 8 the weights are multiples of 1/16."""
    return _tok(F.interpolate(_nchw(x, B, h, w), size=(H, W), mode='bilinear', align_corners=False))


def bilinear_bwd_ref(dout, B, h, w, C, H, W):
    xn = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(xn, size=(H, W), mode='bilinear', align_corners=False).backward(_nchw(dout, B, H, W))
    return _tok(xn.grad)


# ---- known-answer attention -------------------------------------------------------------------------------------------------------
def key_code(Nkv, hd):
    """[Nkv][hd]: the +-1 binary code of the key index (nb = ceil(log2 Nkv) bits, repeated hd // nb times, the rest zero) times 10."""
    nb = max(1, math.ceil(math.log2(Nkv)))
    reps = hd // nb
    assert reps >= 1, (Nkv, hd)
    j = torch.arange(Nkv)
    bits = torch.stack([((j >> b) & 1) for b in range(nb)], 1).double() * 2 - 1          # [Nkv][nb]
    code = torch.zeros(Nkv, hd, dtype=torch.float64)
    code[:, :nb * reps] = bits.repeat(1, reps)
    return code * 10.0, nb, reps


def selector_margin(Nkv, hd, scale):
    """Smallest gap between the scaled score of the chosen key and any other: two keys differ in >= 1 bit of every repetition."""
    _, nb, reps = key_code(Nkv, hd)
    return 100.0 * reps * 2 * scale


def selector_map(B, heads, N, Nkv, g, key_tile=32):
    """pi [B][heads][N]: random, but the first queries and the last ones of every (batch, head) hit the first and last key and the keys on
    each side of every key-tile boundary."""
    pi = torch.randint(0, Nkv, (B, heads, N), generator=g)
    must = sorted({0, Nkv - 1} | {j for t in range(key_tile, Nkv, key_tile) for j in (t - 1, t)})
    must = torch.tensor(must)[:N // 2]
    if must.numel():
        pi[:, :, :must.numel()] = must
        pi[:, :, N - must.numel():] = must.flip(0)
    return pi


def selector_inputs(B, heads, N, Nkv, hd, g, key_tile=32):
    """(q [B N][heads hd], k, v [B Nkv][heads hd], d_o [B N][heads hd], pi) in float64, all exact in bf16."""
    code, _, _ = key_code(Nkv, hd)
    pi = selector_map(B, heads, N, Nkv, g, key_tile)
    k = code[None, :, None, :].expand(B, Nkv, heads, hd).reshape(B * Nkv, heads * hd).clone()
    q = code[pi].permute(0, 2, 1, 3).reshape(B * N, heads * hd).clone()                  # [B][heads][N][hd] -> [B][N][heads][hd]
    v = lattice((B * Nkv, heads * hd), g)
    d_o = lattice((B * N, heads * hd), g)
    return q, k, v, d_o, pi


def selector_answers(v, d_o, pi, B, heads, N, Nkv, hd):
    """Closed form: O[i] = V[pi(i)]; dQ = 0; dK = 0; dV[j] = sum of dO[i] over pi(i) = j."""
    v4 = v.reshape(B, Nkv, heads, hd).permute(0, 2, 1, 3)                                # [B][heads][Nkv][hd]
    o = torch.gather(v4, 2, pi[..., None].expand(B, heads, N, hd))
    do4 = d_o.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    dv = torch.zeros(B, heads, Nkv, hd, dtype=torch.float64)
    dv.scatter_add_(2, pi[..., None].expand(B, heads, N, hd), do4)
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(B * n, heads * hd)                 # noqa: E731
    return back(o, N), torch.zeros(B * N, heads * hd, dtype=torch.float64), torch.zeros(B * Nkv, heads * hd, dtype=torch.float64), back(dv, Nkv)


def uniform_inputs(B, heads, N, Nkv, hd, g):
    """(q = 0, k, v) with lattice k and v.  No column of v sums to zero over the keys of an image (the first key's element is moved to a
    neighbouring lattice value where it would): an exact zero has no last place to be one unit away from."""
    q = torch.zeros(B * N, heads * hd, dtype=torch.float64)
    k, v = lattice((B * Nkv, heads * hd), g), lattice((B * Nkv, heads * hd), g)
    v3 = v.reshape(B, Nkv, heads * hd)
    zero = v3.sum(1) == 0
    first = v3[:, 0]
    first[zero] = torch.where(first[zero] == 3, first[zero] - 1, torch.where(first[zero] == -1, first[zero] + 2, first[zero] + 1))
    assert not (v3.sum(1) == 0).any() and not (v == 0).any()
    return q, k, v


def uniform_answer(v, B, heads, N, Nkv, hd):
    """O = sum(V) / Nkv for every query (float64; exact in every format when Nkv is a power of two)."""
    s = v.reshape(B, Nkv, heads * hd).sum(1) / Nkv
    return s[:, None, :].expand(B, N, heads * hd).reshape(B * N, heads * hd)


def attention_fp32(q, k, v, B, heads, N, Nkv, hd, scale):
    """Plain fp32 softmax attention of torch on the CPU ([B N][heads hd] rows), with autograd: the 'reference alone' check."""
    f = lambda t, n: t.float().reshape(B, n, heads, hd).permute(0, 2, 1, 3)               # noqa: E731
    s = (f(q, N) @ f(k, Nkv).transpose(-1, -2)) * scale
    o = torch.softmax(s, -1) @ f(v, Nkv)
    return o.permute(0, 2, 1, 3).reshape(B * N, heads * hd)
