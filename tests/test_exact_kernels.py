"""Exact known-answer tests of the matrix and attention kernels: inputs for which the right result does not depend on the summation order
(tests/exact_inputs.py), so the tolerance is ZERO by derivation and every tile shape, split-K count, XCD mapping and MFMA form must return
the same bits.  The parity tests of tests/test_kernels_gpu.py bound the largest error by 3 % (and more on gradients) of the largest element
of the tensor; a dropped K element, a K slab counted twice, a truncating store or a bf16 partial sum all pass there and all fail here.

* fp32 outputs: `torch.equal` with the float64 result; bf16 outputs: the raw 16-bit words of that result rounded once to nearest even.
* The only comparison that is not bit equality: uniform attention with a key count that is not a power of two (1 / Nkv is not exact), one
  unit in the last place of the output type against the correctly rounded value.  The only known answer that a documented option makes
  inexact: selector dV under SEGFAC_ATTN64_PRESCALE (derivation in run_attention); the uniform dV is compared there instead.
* Every GPU case is a row of tests/golden/dispatch_table.json -- the row's own entry point, feature sizes, strides, pointer alignments and
  split count; only the token / batch dimension is reduced, by halving, while a dry run still names the row's kernels -- and asserts with
  hip.trace() that those kernels are the ones that ran.  CASES is a greedy cover of every (entry point, kernel) pair of EXACT_PAIRS.

(entry point, kernel) pairs of the table that have no exact test: none (EXCLUDED is empty).

Beside the table: products whose feature sizes N and K are one more and one less than a tile multiple (test_exact_feature_ragged_gemm),
and the depthwise 7 x 7 / 3 x 3 convolutions, the bilinear resize by 2 / 4 / 8 and the column sum (test_exact_spatial_kernels).  The
depthwise convolutions then run in EVERY form of csrc/conv.hip (strip, vertical walk with its row switch, one-launch; 3 x 3 forward
included) at the shapes where their dispatch changes (test_exact_depthwise_forms, test_exact_depthwise7_shapes; the shape tables are those
of tests/dwconv_refs.py), and one sampled 67 M-element map reaches the second strip of a dwconv7x7_kernel thread
(test_exact_depthwise7_second_strip_of_a_thread).  Not covered for the depthwise family: the weight gradient at that size, the block caps
of the three weight-gradient plans and the walk kernel's own grid-stride loop.

Not covered by this module: kernels with a division or a transcendental.  Of those the norms and the column reductions (LayerNorm,
BatchNorm, GRN, colsum) are checked against float64 in tests/test_norm_float64.py, and GELU and its derivative inside the depthwise
kernels in tests/test_dwconv_float64.py; softmax-CE and fp8 quantisation keep their tolerance tests.  The bilinear backward and fused forms (bilinear_bwd and its
integer-ratio kernels, bilinear_bwd_248 on the VALU and on the matrix pipe, upsample_add (+ statistics), fuse_map_248), adaptive_avgpool
and nearest_up are checked bit for bit on lattice inputs, and per element against float64 on other inputs, in tests/test_resize_float64.py
(references: tests/resize_refs.py).  The pure data movers im2col, col2im, permute021 and cast2d keep their tolerance tests: no reference yet.
"""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

import exact_inputs as X

BF, F32 = torch.bfloat16, torch.float32
# (segf_conv3x3_fwd_splitk, the eighth entry point the issue names, is a host query: it launches nothing and has no row in the table)
FNS = ('segf_gemm', 'segf_gemm_pro', 'segf_conv3x3', 'segf_gemm_dw_db', 'segf_gemm_dw_db_grouped', 'segf_attention_fwd',
       'segf_attention_bwd')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# Every (entry point, kernel) pair of the eight entry points in tests/golden/dispatch_table.json (fp8 configurations not counted) that an
# exact GPU test below runs and names in its trace assertion.  test_every_table_pair_is_listed walks the table against this list.
EXACT_PAIRS = '''
segf_attention_bwd|attn_bwd_dq64p_kernel<QW, false>
segf_attention_bwd|attn_dkv_reduce_kernel<bf16_t>
segf_attention_bwd|attn_mfma_bwd_dkv_kernel<64, false, true, true, 2, 128>
segf_attention_bwd|attn_mfma_bwd_fused_kernel<32, 4>
segf_attention_fwd|attn_fwd64p_kernel<QW, false>
segf_attention_fwd|attn_mfma_fwd_kernel<32, QW, false, 4, false>
segf_conv3x3|gemm8_kernel<0, 0, true, 0, bf16_t>
segf_conv3x3|gemm8_kernel<0, 0, true, 0, float>
segf_conv3x3|gemm8_kernel<1, 1, true, 0, float>
segf_conv3x3|gemm_bf16_big_kernel<0, bf16_t, true>
segf_conv3x3|gemm_bf16_kernel<2, float, true, true>
segf_conv3x3|splitk_reduce_wide_kernel<OutT> [OutT = float]
segf_conv3x3|splitk_reduce_wide_kernel<OutT> [OutT = unsigned short]
segf_gemm|gemm8_kernel<0, 0, false, 0, bf16_t>
segf_gemm|gemm8_kernel<0, 1, false, 0, bf16_t>
segf_gemm|gemm8_kernel<1, 1, false, 0, float>
segf_gemm|gemm_bf16_big_kernel<0, bf16_t, false, false, 1, true>
segf_gemm|gemm_bf16_big_kernel<0, bf16_t, false, false, 1>
segf_gemm|gemm_bf16_big_kernel<0, bf16_t, false>
segf_gemm|gemm_bf16_big_kernel<1, bf16_t, false, false, 1>
segf_gemm|gemm_bf16_big_kernel<1, bf16_t, false>
segf_gemm|gemm_bf16_big_kernel<2, float, false>
segf_gemm|gemm_bf16_kernel<(0 == 2 ? 0 : 0), bf16_t, true, false, 1>
segf_gemm|gemm_bf16_kernel<(0 == 2 ? 0 : 0), float, true, false, 1>
segf_gemm|gemm_bf16_kernel<(1 == 2 ? 0 : 1), bf16_t, true, false, 1>
segf_gemm|gemm_bf16_kernel<0, bf16_t, true, false, 2, true>
segf_gemm|gemm_bf16_kernel<0, float, true, false, 2, true>
segf_gemm|gemm_bf16_kernel<1, bf16_t, true, false, 2, true>
segf_gemm|gemm_bf16_kernel<1, float, true, false, 2, true>
segf_gemm|gemm_bf16_kernel<2, float, true, false, 2, true>
segf_gemm|gemm_skinny_k_kernel<LAYOUT, 2, NT> [LAYOUT = 0, NT = 4]
segf_gemm|gemm_skinny_k_kernel<LAYOUT, 2, NT> [LAYOUT = 1, NT = 4]
segf_gemm|gemm_skinny_k_kernel<LAYOUT, 6, NT> [LAYOUT = 1, NT = 2]
segf_gemm|gemm_skinny_k_kernel<LAYOUT, 6, NT> [LAYOUT = 1, NT = 4]
segf_gemm|gemm_skinny_kernel<LAYOUT, 1, 2> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 1, 2> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 1, 4> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 1, 8> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 1, 8> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 2, 2> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 2, 4> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 2, 4> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 2, 8> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 2, 8> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 4, 2> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 4, 2> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 4, 4> [LAYOUT = 0]
segf_gemm|gemm_skinny_kernel<LAYOUT, 4, 4> [LAYOUT = 1]
segf_gemm|gemm_skinny_kernel<LAYOUT, 5, 2> [LAYOUT = 0]
segf_gemm|splitk_reduce4_kernel [OutT = float]
segf_gemm|splitk_reduce_wide_kernel<OutT> [OutT = float]
segf_gemm_dw_db|colreduce_finalize_kernel
segf_gemm_dw_db|colreduce_kernel<NOUT, F> [NOUT = 1, F = ColsumF<unsigned short>]
segf_gemm_dw_db|gemm_bf16_big_kernel<2, float, false, false, 2>
segf_gemm_dw_db|gemm_bf16_big_kernel<2, float, false>
segf_gemm_dw_db|gemm_bf16_kernel<2, float, true, false, 2, true>
segf_gemm_dw_db|splitk_reduce4_kernel [OutT = float]
segf_gemm_dw_db|splitk_reduce_wide_kernel<OutT> [OutT = float]
segf_gemm_dw_db_grouped|colreduce_finalize_kernel
segf_gemm_dw_db_grouped|colreduce_kernel<NOUT, F> [NOUT = 1, F = ColsumF<unsigned short>]
segf_gemm_dw_db_grouped|gemm8_kernel<1, 1, false, 0, float>
segf_gemm_dw_db_grouped|gemm_bf16_big_kernel<2, float, false>
segf_gemm_dw_db_grouped|gemm_bf16_dw_group_kernel<true>
segf_gemm_dw_db_grouped|gemm_bf16_kernel<2, float, true, false, 2, true>
segf_gemm_dw_db_grouped|gemm_bf16_kernel<2, float, true>
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 10, true> [MT = 2]
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 2, true> [MT = 2]
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 2, true> [MT = 4]
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 2, true> [MT = 8]
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 4, true> [MT = 4]
segf_gemm_dw_db_grouped|gemm_dw_skinny_kernel<MT, 8, true> [MT = 2]
segf_gemm_dw_db_grouped|splitk_reduce_group_kernel
segf_gemm_pro|gemm_bf16_big_kernel<0, bf16_t, false, true, 1, true>
'''
EXACT_PAIRS = [tuple(l.split('|', 1)) for l in EXACT_PAIRS.strip().split('\n')]
EXCLUDED = {}          # (entry point, kernel) -> the reason it cannot have an exact test; at most one fifth of the pairs


# ---- the table and the cases ------------------------------------------------------------------------------------------------------
def _table_entries():
    with open(os.path.join(GOLDEN, 'dispatch_table.json')) as fh:
        table = json.load(fh)
    out = []
    for cfg in sorted(table):
        if cfg.endswith('_fp8'):
            continue
        out += [(cfg, e) for e in table[cfg] if e['fn'] in FNS]
    return out


def _tokens(e):
    """Size of the dimension a case may reduce (tokens / images): the cheapest row of a kernel form is chosen by it."""
    fn, a = e['fn'], e['args']
    if fn in ('segf_gemm', 'segf_gemm_pro'):
        return a[4] if a[1] == 2 else a[2]
    if fn == 'segf_gemm_dw_db':
        return a[3]
    if fn == 'segf_gemm_dw_db_grouped':
        return sum(it[2] * it[0] * it[1] for it in a[1]) >> 16
    if fn == 'segf_conv3x3':
        return a[1] * a[2] * a[3] * a[4] * a[5] >> 10
    return a[1] * a[2] * a[3]


def _cases():
    """Greedy cover of EXACT_PAIRS by table rows (deterministic: most uncovered pairs first, then the cheapest row, then table order)."""
    want, seen, rows = set(EXACT_PAIRS), set(), []
    for cfg, e in _table_entries():
        key = (e['fn'], json.dumps(e['args']))
        if key not in seen:
            seen.add(key)
            rows.append((cfg, e))
    cases = []
    # rows of at most 2^18 tokens first (their operands and float64 references stay small); the rest only for what those leave uncovered
    for limit in (1 << 18, None):
        while want:
            best, gain = None, 0
            for i, (cfg, e) in enumerate(rows):
                if limit and _max_tokens(e) > limit:
                    continue
                g = len({(e['fn'], k) for k in e['kernels']} & want)
                if g > gain or (g == gain and g and _tokens(e) < _tokens(rows[best][1])):
                    best, gain = i, g
            if best is None:
                break                                        # a listed pair that no row has: test_every_table_pair_is_listed fails
            cfg, e = rows.pop(best)
            new = {(e['fn'], k) for k in e['kernels']} & want
            want -= new
            cases.append((cfg, dict(e, targets=sorted(k for _, k in new))))
    return cases


def _max_tokens(e):
    a = e['args']
    if e['fn'] == 'segf_gemm_dw_db_grouped':
        return max(it[2] for it in a[1])
    return a[1] * a[2] * a[3] if e['fn'] == 'segf_conv3x3' else _tokens(e)


CASES = _cases()
CASE_IDS = ['%02d-%s-%s' % (i, e['fn'][5:], cfg) for i, (cfg, e) in enumerate(CASES)]


def _with(e, **kw):
    """Copy of a table row with some arguments replaced (by position name of its entry point)."""
    fn, a = e['fn'], list(e['args'])
    pos = {'segf_gemm': dict(M=2, N=3, K=4, split_k=17, ws=18), 'segf_gemm_pro': dict(M=2, N=3, K=4, split_k=13, ws=14),
           'segf_gemm_dw_db': dict(M=1, N=2, K=3, split_k=11), 'segf_conv3x3': dict(B=1, H=2, W=3, split_k=14, ws=15),
           'segf_attention_fwd': dict(B=1, N=3, Nkv=4), 'segf_attention_bwd': dict(B=1, N=3, Nkv=4)}
    if fn == 'segf_gemm_dw_db_grouped':
        items = [list(it) for it in a[1]]
        for it in items:
            it[2] += kw.get('dK', 0)
        a[1] = items
    else:
        for k, v in kw.items():
            a[pos[fn][k]] = v
    return dict(e, args=a)


def _dry(e):
    """Kernels a dry run of the call names, or None when the entry point refuses the arguments (a non-zero return code).  A missing
    library is an error of its own, raised by hip.lib() here."""
    from segmentation_factory_amd import dispatch, hip
    hip.lib()
    try:
        return dispatch.replay(e)
    except RuntimeError as err:
        if 'in a dry run' not in str(err):
            raise
        return None


def _token_dim(e):
    """(name of the reducible dimension, its value, the floor below which a case is not reduced)."""
    fn, a = e['fn'], e['args']
    if fn == 'segf_gemm':
        rpg = a[16] if a[15] is not None else 1
        return ('K', a[4], 2048) if a[1] == 2 else ('M', a[2], max(1024, 2 * rpg))
    if fn == 'segf_gemm_pro':
        return ('K', a[4], 2048) if a[1] == 2 else ('M', a[2], max(1024, 2 * a[17]))
    if fn == 'segf_gemm_dw_db':
        return 'K', a[3], 2048
    if fn == 'segf_conv3x3':
        return 'B', a[1], 1
    return 'B', a[1], 1


def reduce_case(e):
    """The row with its token / batch dimension halved as long as a dry run names the row's kernels (attention: the images, then the
    queries).  The feature sizes, strides, alignments and split count are the row's."""
    want = e['kernels']
    if e['fn'] == 'segf_gemm_dw_db_grouped':
        # the 'batch' of a grouped call is its members and their token counts: members are dropped and token counts halved while the
        # kernels this case is listed for (e['targets']) are all named and no kernel outside the row's is
        same = lambda items: _same_kernels(e, _dry(dict(e, args=[e['args'][0], items])))   # noqa: E731
        items = [list(it) for it in e['args'][1]]
        k = len(items) - 1
        while k >= 0:
            if len(items) > 1 and same(items[:k] + items[k + 1:]):
                del items[k]
            k -= 1
        for it in items:
            while it[2] % 2 == 0 and it[2] // 2 >= 1024:
                it[2] //= 2
                if not same(items):
                    it[2] *= 2
                    break
        return dict(e, args=[e['args'][0], items])
    name, v, floor = _token_dim(e)
    while v % 2 == 0 and v // 2 >= floor and _dry(_with(e, **{name: v // 2})) == want:
        v //= 2
    e = _with(e, **{name: v})
    if e['fn'].startswith('segf_attention'):
        n = e['args'][3]
        while n % 2 == 0 and n // 2 >= 512 and _dry(_with(e, N=n // 2)) == want:
            n //= 2
        e = _with(e, N=n)
    return e


def ragged_neighbours(e):
    """Ragged neighbours of a reduced case that the same kernels take (dry run): the token dimension one more and one less than the case's
    (a tile multiple in every row of the table); attention: queries and keys one less; conv: an odd image height and width."""
    fn, a, out = e['fn'], e['args'], []
    if fn == 'segf_gemm_dw_db_grouped':
        cand = [_with(e, dK=1), _with(e, dK=-1)]
        if not any(_same_kernels(e, _dry(c)) for c in cand):              # kernels that take whole 32-token groups only
            cand = [_with(e, dK=32), _with(e, dK=-32)]
    elif fn.startswith('segf_attention'):
        cand = [_with(e, N=a[3] - 1), _with(e, N=a[3] + 1), _with(e, Nkv=a[4] - 1), _with(e, N=a[3] - 3, Nkv=a[4] - 5)]
    elif fn == 'segf_conv3x3':
        cand = [_with(e, H=a[2] - 1, W=a[3] - 1), _with(e, H=a[2] + 1, W=a[3] - 1), _with(e, W=a[3] - 1)]
    else:
        name, v, _ = _token_dim(e)
        cand = [_with(e, **{name: v + 1}), _with(e, **{name: v - 1})]
    for c in cand:
        if _same_kernels(e, _dry(c)):
            out.append(c)
    return out


def _same_kernels(e, got):
    """The trace assertion: the row's kernels, in order (grouped weight gradients: every kernel the case is listed for and none that the
    row does not name, see reduce_case)."""
    if got is None:
        return False
    if e['fn'] == 'segf_gemm_dw_db_grouped':
        return set(e['targets']) <= set(got) <= set(e['kernels'])
    return got == e['kernels']


# ---- device buffers: the row's strides and pointer alignments ----------------------------------------------------------------------
SENTINEL = -65536.0


class Buf:
    """A [rows][cols] operand with leading dimension ld whose first element sits `align` bytes past a 256-byte boundary.  Inputs: the pad
    columns hold lattice values, not zeros (a kernel that reads them into a sum is caught).  Outputs: everything is SENTINEL first and
    `untouched()` tells whether the pad columns and the guard band around the buffer still are."""

    def __init__(self, rows, cols, ld, align, dtype, data=None):
        assert ld >= cols, (ld, cols)
        esz = torch.empty(0, dtype=dtype).element_size()
        n = rows * ld
        guard = 256 // esz
        if data is None:
            host = torch.full((n + 3 * guard,), SENTINEL, dtype=dtype)
        else:
            host = torch.full((n + 3 * guard,), 3.0, dtype=dtype)
        probe = torch.empty(n + 3 * guard, dtype=dtype, device='cuda')
        off = guard + ((int(align) - probe.data_ptr()) % 256) // esz
        if data is not None:
            host[off:off + n].view(rows, ld)[:, :cols] = data.to(dtype)
        probe.copy_(host)
        self.raw, self.off, self.n, self.rows, self.cols, self.ld = probe, off, n, rows, cols, ld
        self.t = probe[off:off + n].view(rows, ld)[:, :cols]
        assert self.t.data_ptr() % 256 == int(align) % 256

    @property
    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        h = self.raw.cpu().float()
        inside = torch.zeros(h.numel(), dtype=torch.bool)
        inside[self.off:self.off + self.n].view(self.rows, self.ld)[:, :self.cols] = True
        return bool((h[~inside] == SENTINEL).all())


def _al(p):
    return None if p is None else int(p[1:])


def _dt(code):
    return BF if code == 1 else F32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nfloats):
    return torch.full((max(int(nfloats), 1) + 64,), float('nan'), dtype=F32, device='cuda')


# ---- one row, run with real tensors: returns (trace, [(name, got, float64 reference)], [output buffers]) ---------------------------
def run_gemm(e, seed=1):
    from segmentation_factory_amd import hip
    lib = hip.lib()
    dt, layout, M, N, K, pa, lda, pb, ldb, pc, c_dt, ldc, pbias, pres, ldr, prs, rpg, split_k, pws, _ = e['args']
    assert K < X.FP32_EXACT_TERMS
    g = X.gen(seed)
    (ar, ac), (br, bc) = X.gemm_operand_shapes(layout, M, N, K)
    A64, B64 = X.lattice((ar, ac), g), X.lattice((br, bc), g, pow2=-1)
    A, B = Buf(ar, ac, lda, _al(pa), _dt(dt), A64), Buf(br, bc, ldb, _al(pb), _dt(dt), B64)
    Cb = Buf(M, N, ldc, _al(pc), _dt(c_dt))
    bias64 = X.integers((N,), g) if pbias is not None else None
    res64 = X.lattice((M, N), g) if pres is not None else None
    rs64 = X.pow2s((-(-M // rpg),), g) if prs is not None else None
    bias = None if bias64 is None else Buf(1, N, N, _al(pbias), F32, bias64[None])
    res = None if res64 is None else Buf(M, N, ldr, _al(pres), _dt(dt), res64)
    rs = None if rs64 is None else Buf(1, rs64.numel(), rs64.numel(), _al(prs), F32, rs64[None])
    ws = _ws(split_k * M * N) if pws is not None else None
    p = lambda b: None if b is None else b.ptr                                          # noqa: E731
    with hip.trace() as t:
        rc = lib.segf_gemm(dt, layout, M, N, K, A.ptr, lda, B.ptr, ldb, Cb.ptr, c_dt, ldc, p(bias), p(res), ldr, p(rs), rpg, split_k,
                           None if ws is None else ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return t.kernels, [('C', Cb.t, X.gemm_ref(layout, A64, B64, bias64, res64, rs64, rpg))], [Cb]


def run_gemm_pro(e, seed=2):
    from segmentation_factory_amd import hip
    lib = hip.lib()
    dt, layout, M, N, K, pa, lda, pb, ldb, pc, c_dt, ldc, pbias, split_k, pws, ps, pt, rpg, act, _ = e['args']
    g = X.gen(seed)
    (ar, ac), (br, bc) = X.gemm_operand_shapes(layout, M, N, K)
    A64, B64 = X.lattice((ar, ac), g), X.lattice((br, bc), g)
    tokens, feats = (M, K) if layout == 0 else (K, N)
    groups = -(-tokens // rpg)
    # x s + t with s in {1/2, 1, 2} and integer t: multiples of 1/2 below 9, exact in fp32 and in bf16; ReLU keeps them
    s64, t64 = X.pow2s((groups, feats), g, (-1, 0, 1)), X.integers((groups, feats), g, -2, 2)
    bias64 = X.integers((N,), g) if pbias is not None else None
    A, B = Buf(ar, ac, lda, _al(pa), _dt(dt), A64), Buf(br, bc, ldb, _al(pb), _dt(dt), B64)
    Cb = Buf(M, N, ldc, _al(pc), _dt(c_dt))
    bias = None if bias64 is None else Buf(1, N, N, _al(pbias), F32, bias64[None])
    sc, sh = Buf(groups, feats, feats, _al(ps), F32, s64), Buf(groups, feats, feats, _al(pt), F32, t64)
    ws = _ws(split_k * M * N) if pws is not None else None
    with hip.trace() as t:
        rc = lib.segf_gemm_pro(dt, layout, M, N, K, A.ptr, lda, B.ptr, ldb, Cb.ptr, c_dt, ldc, None if bias is None else bias.ptr, split_k,
                               None if ws is None else ws.data_ptr(), sc.ptr, sh.ptr, rpg, act, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return t.kernels, [('C', Cb.t, X.gemm_pro_ref(layout, A64, B64, s64, t64, rpg, act, bias64))], [Cb]


def run_dw_db(e, seed=3):
    from segmentation_factory_amd import hip
    lib = hip.lib()
    dt, M, N, K, pa, lda, pb, ldb, pc, c_dt, ldc, split_k, pws, pdb, _ = e['args']
    assert K < X.FP32_EXACT_TERMS
    g = X.gen(seed)
    dy64, x64 = X.lattice((K, M), g), X.lattice((K, N), g, pow2=1)
    dy, x = Buf(K, M, lda, _al(pa), _dt(dt), dy64), Buf(K, N, ldb, _al(pb), _dt(dt), x64)
    dw, db = Buf(M, N, ldc, _al(pc), _dt(c_dt)), Buf(1, M, M, _al(pdb), F32)
    ws = _ws(lib.segf_gemm_dw_db_ws(M, N, K, split_k))
    with hip.trace() as t:
        rc = lib.segf_gemm_dw_db(dt, M, N, K, dy.ptr, lda, x.ptr, ldb, dw.ptr, c_dt, ldc, split_k, ws.data_ptr(), db.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    rw, rb = X.dw_db_ref(dy64, x64)
    return t.kernels, [('dw', dw.t, rw), ('db', db.t[0], rb)], [dw, db]


def run_dw_db_grouped(e, seed=4):
    from segmentation_factory_amd import hip
    lib = hip.lib()
    dt, desc = e['args']
    g = X.gen(seed)
    arr = (hip.SegfDwItem * len(desc))()
    keep, outs, bufs = [], [], []
    for k, (M, N, K, lddy, ldx, lddw, split_k, shared) in enumerate(desc):
        assert K < X.FP32_EXACT_TERMS
        dy64, x64 = X.lattice((K, M), g), X.lattice((K, N), g)
        dy, x = Buf(K, M, lddy, 0, _dt(dt), dy64), Buf(K, N, ldx, 0, _dt(dt), x64)
        dw, db = Buf(M, N, lddw, 0, F32), Buf(1, M, M, 0, F32)
        ws = _ws(lib.segf_gemm_dw_db_ws(M, N, K, split_k))
        keep += [dy, x, ws]
        it = arr[k]
        it.M, it.N, it.K, it.lddy, it.ldx, it.lddw, it.split_k, it.shared_split = M, N, K, lddy, ldx, lddw, split_k, shared
        it.dy, it.x, it.dw, it.db, it.ws = dy.ptr, x.ptr, dw.ptr, db.ptr, ws.data_ptr()
        outs.append((dw, db, dy64, x64))
        bufs += [dw, db]
    with hip.trace() as t:
        rc = lib.segf_gemm_dw_db_grouped(dt, len(desc), C.cast(arr, C.c_void_p), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    res = []
    for k, (dw, db, dy64, x64) in enumerate(outs):
        rw, rb = X.dw_db_ref(dy64, x64)
        res += [(f'item {k} {desc[k][:3]} dw', dw.t, rw), (f'item {k} {desc[k][:3]} db', db.t[0], rb)]
    return t.kernels, res, bufs


def run_conv3x3(e, seed=5):
    from segmentation_factory_amd import hip
    lib = hip.lib()
    mode, B, H, W, Cin, Cout, px, ldx, pw, ldw, py, y_dt, ldy, pbias, split_k, pws, _ = e['args']
    P = B * H * W
    assert 9 * max(Cin, Cout) < X.FP32_EXACT_TERMS and P < X.FP32_EXACT_TERMS
    g = X.gen(seed)
    xs, wsz, ys = {0: ((P, Cin), (Cout, 9 * Cin), (P, Cout)), 1: ((P, Cout), (Cin, 9 * Cout), (P, Cin)),
                   2: ((P, Cin), (P, Cout), (Cout, 9 * Cin))}[mode]
    x64, w64 = X.lattice(xs, g), X.lattice(wsz, g, pow2=-2)
    bias64 = X.integers((Cout,), g) if pbias is not None else None
    x, w = Buf(*xs, ldx, _al(px), BF, x64), Buf(*wsz, ldw, _al(pw), BF, w64)
    y = Buf(*ys, ldy, _al(py), _dt(y_dt))
    bias = None if bias64 is None else Buf(1, Cout, Cout, _al(pbias), F32, bias64[None])
    ws = _ws(split_k * ys[0] * ys[1]) if pws is not None else None
    with hip.trace() as t:
        rc = lib.segf_conv3x3(mode, B, H, W, Cin, Cout, x.ptr, ldx, w.ptr, ldw, y.ptr, y_dt, ldy, None if bias is None else bias.ptr,
                              split_k, None if ws is None else ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return t.kernels, [('y', y.t, X.conv3x3_ref(mode, x64, w64, B, H, W, Cin, Cout, bias64))], [y]


def run_attention(e, family, seed=6):
    """Forward (and, for a segf_attention_bwd row, the backward on the forward's own o and lse) on selector or uniform inputs."""
    from segmentation_factory_amd import hip
    lib = hip.lib()
    a = e['args']
    bwd = e['fn'] == 'segf_attention_bwd'
    dt, B, heads, N, Nkv, hd, pq, ldq, pk, ldk, pv, ldv, scale = a[:13]
    po, ldo = a[13], a[14]
    g = X.gen(seed)
    D = heads * hd
    if family == 'selector':
        q64, k64, v64, do64, pi = X.selector_inputs(B, heads, N, Nkv, hd, g)
        assert X.selector_margin(Nkv, hd, scale) > 110          # exp(-104) is below the smallest fp32 denormal: the other keys are exactly 0
        o64, dq64, dk64, dv64 = X.selector_answers(v64, do64, pi, B, heads, N, Nkv, hd)
    else:
        q64, k64, v64 = X.uniform_inputs(B, heads, N, Nkv, hd, g)
        o64 = X.uniform_answer(v64, B, heads, N, Nkv, hd)
    q, k, v = Buf(B * N, D, ldq, _al(pq), _dt(dt), q64), Buf(B * Nkv, D, ldk, _al(pk), _dt(dt), k64), \
        Buf(B * Nkv, D, ldv, _al(pv), _dt(dt), v64)
    o = Buf(B * N, D, ldo, _al(po), _dt(dt))
    lse = torch.empty(B * heads * N, dtype=F32, device='cuda')
    with hip.trace() as tf:
        rc = lib.segf_attention_fwd(dt, B, heads, N, Nkv, hd, q.ptr, ldq, k.ptr, ldk, v.ptr, ldv, scale, o.ptr, ldo, lse.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ulp = 0 if (family == 'selector' or Nkv & (Nkv - 1) == 0) else 1          # 1 / Nkv is exact only for a power of two
    res = [(f'{family} O', o.t, o64, ulp)]
    if not bwd:
        return tf.kernels, res, [o]
    X.assert_exact(o.t, o64, 'forward O in front of the backward', ulp)
    if family == 'uniform':
        do64 = X.lattice((B * N, D), g)
    pdo, lddo, plse, pdq, lddq, pdk, lddk, pdv, lddv = a[15], a[16], a[17], a[18], a[19], a[20], a[21], a[22], a[23]
    d_o = Buf(B * N, D, lddo, _al(pdo), _dt(dt), do64)
    dq, dk, dv = Buf(B * N, D, lddq, _al(pdq), _dt(dt)), Buf(B * Nkv, D, lddk, _al(pdk), _dt(dt)), Buf(B * Nkv, D, lddv, _al(pdv), _dt(dt))
    ws = _ws(lib.segf_attention_bwd_ws(B, heads, N, Nkv, hd))
    with hip.trace() as t:
        rc = lib.segf_attention_bwd(dt, B, heads, N, Nkv, hd, q.ptr, ldq, k.ptr, ldk, v.ptr, ldv, scale, o.ptr, ldo, d_o.ptr, lddo,
                                    lse.data_ptr(), dq.ptr, lddq, dk.ptr, lddk, dv.ptr, lddv, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    if family == 'uniform':
        # P = exp(0 - lse) = (1 / Nkv) (1 + a few fp32 roundings), rounded to bf16 for the matrix pipe: exactly 1 / Nkv for a power of two.
        # dV = P^T dO does not depend on o: dV[j] = sum_i dO[i] / Nkv for every key, exact.  (dQ and dK go through dP - D with the ROUNDED o
        # and a bf16 dS: not exact, not compared.)
        assert Nkv & (Nkv - 1) == 0
        dv64 = (do64.reshape(B, N, D).sum(1) / Nkv)[:, None, :].expand(B, Nkv, D).reshape(B * Nkv, D)
        return t.kernels, [('uniform dV', dv.t, dv64, 0)], [dq, dk, dv]
    res = [('selector dQ', dq.t, dq64, 0), ('selector dK', dk.t, dk64, 0)]
    if not (hip.policy('SEGFAC_ATTN64_PRESCALE') and hd == 64 and Nkv >= 128):
        res.append(('selector dV', dv.t, dv64, 0))
    # SEGFAC_ATTN64_PRESCALE (include/segfac.h): the forward and the query-side backward score with bf16(q c), c = scale log2 e, the key-side
    # backward with q c.  Every selector query element is +-10, so the two scores of the chosen key differ by the ONE relative rounding d
    # of bf16(10 c), |d| <= 2^-9, times a score of 100 (hd // nb) nb c ~ 10^3: the key-side kernel's P = exp2(-score d) is a constant
    # anywhere in [1/4, 4], not 1, and selector dV = P sum dO is not a known answer under the option (dS = P (dP - D) = P * 0 still is: dQ
    # and dK stay exactly 0).  Under the option dV is pinned by the uniform family instead (Q = 0 has no rounding to differ by).
    return t.kernels, res, [dq, dk, dv]


def run_case(e):
    """Run one (reduced) row; assert that its outputs are exact and nothing outside them was written.  Returns the kernels that ran."""
    fn = e['fn']
    if fn.startswith('segf_attention'):
        kernels = None
        nkv = e['args'][4]
        for family in (('selector', 'uniform') if not fn.endswith('bwd') or nkv & (nkv - 1) == 0 else ('selector',)):
            kernels, res, bufs = run_attention(e, family)
            for name, got, ref, ulp in res:
                X.assert_exact(got, ref, f'{fn} {e["args"][:6]} {name}', ulp)
            assert all(b.untouched() for b in bufs), f'{fn}: wrote outside its output'
        return kernels
    run = {'segf_gemm': run_gemm, 'segf_gemm_pro': run_gemm_pro, 'segf_gemm_dw_db': run_dw_db, 'segf_gemm_dw_db_grouped': run_dw_db_grouped,
           'segf_conv3x3': run_conv3x3}[fn]
    kernels, res, bufs = run(e)
    for name, got, ref in res:
        X.assert_exact(got, ref, f'{fn} {[a for a in e["args"] if not isinstance(a, list)][:6]} {name}')
    assert all(b.untouched() for b in bufs), f'{fn}: wrote outside its output (pad columns or guard band)'
    return kernels


# =================================================== CPU: the table against the list =================================================
def test_every_table_pair_is_listed():
    """Every (entry point, kernel) pair of the eight entry points in tests/golden/dispatch_table.json (fp8 configurations aside) is in
    EXACT_PAIRS -- and then in the trace assertion of a CASE -- or in EXCLUDED with its reason; at most a fifth may be excluded."""
    pairs = {(e['fn'], k) for _, e in _table_entries() for k in e['kernels']}
    assert len(pairs) >= 60
    listed, excl = set(EXACT_PAIRS), set(EXCLUDED)
    assert not (listed & excl)
    assert pairs - listed - excl == set(), sorted(pairs - listed - excl)
    assert (listed | excl) - pairs == set(), sorted((listed | excl) - pairs)          # a stale entry
    assert len(excl) * 5 <= len(pairs) and all(EXCLUDED.values())
    covered = {(e['fn'], k) for _, e in CASES for k in e['targets']}
    assert listed <= covered, sorted(listed - covered)
    assert len(CASES) == len(CASE_IDS) == len(set(CASE_IDS))


def test_cases_reduce_to_the_same_kernels():
    """Dry runs (no GPU): every case, reduced, still names its row's kernels, keeps the row's feature sizes and stays inside the range in
    which lattice sums are exact in fp32; the largest weight-gradient case keeps >= 65536 pixels on the eight-phase kernel."""
    biggest_dw8 = 0
    for cfg, e in CASES:
        r = reduce_case(e)
        assert _same_kernels(e, _dry(r)), (cfg, e['fn'], r['args'])
        if e['fn'] == 'segf_gemm_dw_db_grouped':
            assert all(any(it[:2] + it[3:] == jt[:2] + jt[3:] for jt in e['args'][1]) for it in r['args'][1])
            if 'gemm8_kernel<1, 1, false, 0, float>' in e['kernels']:
                biggest_dw8 = max(biggest_dw8, max(it[2] for it in r['args'][1]))
            assert max(it[2] for it in r['args'][1]) < X.FP32_EXACT_TERMS
        elif e['fn'] in ('segf_gemm', 'segf_gemm_pro', 'segf_gemm_dw_db'):
            assert r['args'][4 if e['fn'] != 'segf_gemm_dw_db' else 3] < X.FP32_EXACT_TERMS
    assert biggest_dw8 >= 65536, biggest_dw8


# =================================================== CPU: the references alone, and their mutants ====================================
def _gemm_problem(layout, M, N, K, seed, epilogue=True):
    g = X.gen(seed)
    (ar, ac), (br, bc) = X.gemm_operand_shapes(layout, M, N, K)
    A, B = X.lattice((ar, ac), g), X.lattice((br, bc), g, pow2=-1)
    if not epilogue:
        return A, B, None, None, None, 1
    return A, B, X.integers((N,), g), X.lattice((M, N), g), X.pow2s((-(-M // 100),), g), 100


def _gemm_fp32(layout, A, B, bias, res, rs, rpg):
    A, B = A.float(), B.float()
    v = A @ B.t() if layout == 0 else A @ B if layout == 1 else A.t() @ B
    if bias is not None:
        v = v + bias.float()[None]
    if res is not None:
        v = res.float() + rs.float()[torch.arange(v.shape[0]) // rpg][:, None] * v
    return v


def test_references_equal_torch_fp32_on_lattice_inputs():
    """The condition 'the reference alone passes': torch's own fp32 CPU op on the same inputs equals every float64 reference exactly (and,
    stored as bf16, equals it rounded once), through the comparison function the GPU tests use."""
    for layout in (0, 1, 2):
        p = _gemm_problem(layout, 513, 259, 1031, 10 + layout)
        ref = X.gemm_ref(layout, *p)
        got = _gemm_fp32(layout, *p)
        X.assert_exact(got, ref, f'gemm layout {layout} fp32')
        X.assert_exact(got.to(BF), ref, f'gemm layout {layout} bf16')
    g = X.gen(20)
    dy, x = X.lattice((131072, 64), g), X.lattice((131072, 96), g, pow2=1)           # the 131072-pixel weight gradient
    rw, rb = X.dw_db_ref(dy, x)
    X.assert_exact(dy.float().t() @ x.float(), rw, 'dw')
    X.assert_exact(dy.float().sum(0), rb, 'db')
    X.assert_exact(dy[:65536].float().t() @ x[:65536].float() + dy[65536:].float().t() @ x[65536:].float(), rw, 'dw as two K halves')
    # segf_gemm_pro: the normalised operand
    A, B = X.lattice((200, 48), g), X.lattice((24, 48), g)
    s, t = X.pow2s((2, 48), g, (-1, 0, 1)), X.integers((2, 48), g, -2, 2)
    gi = torch.arange(200) // 100
    got = torch.relu(A.float() * s.float()[gi] + t.float()[gi]).to(BF).float() @ B.float().t()
    X.assert_exact(got, X.gemm_pro_ref(0, A, B, s, t, 100, 1), 'gemm_pro')
    # 3x3 conv, NHWC, odd sizes, the input a column slice of a wider buffer
    Bn, H, W, I, O = 2, 5, 7, 16, 24
    wide = X.lattice((Bn * H * W, I + 16), g)
    xt = wide[:, 8:8 + I]
    w4, dy4 = X.lattice((O, I, 3, 3), g, pow2=-2), X.lattice((Bn, O, H, W), g)
    bias = X.integers((O,), g)
    xn = xt.float().reshape(Bn, H, W, I).permute(0, 3, 1, 2).requires_grad_(True)
    wn = w4.float().requires_grad_(True)
    y = F.conv2d(xn, wn, bias.float(), padding=1)
    y.backward(dy4.float())
    tok = lambda t_: t_.permute(0, 2, 3, 1).reshape(-1, t_.shape[1])                    # noqa: E731
    wm, wt = w4.permute(0, 2, 3, 1).reshape(O, 9 * I), w4.permute(1, 2, 3, 0).reshape(I, 9 * O)
    X.assert_exact(tok(y.detach()), X.conv3x3_ref(0, xt, wm, Bn, H, W, I, O, bias), 'conv3x3 forward')
    X.assert_exact(tok(xn.grad), X.conv3x3_ref(1, tok(dy4), wt, Bn, H, W, I, O), 'conv3x3 data gradient')
    X.assert_exact(wn.grad.permute(0, 2, 3, 1).reshape(O, 9 * I), X.conv3x3_ref(2, xt, tok(dy4), Bn, H, W, I, O), 'conv3x3 weight gradient')
    # patch conv = im2col + layout-0 product (stride 4, 7 x 7, pad 3): the column matrix is a data mover, the product is gemm_ref
    xi = X.lattice((2, 3, 16, 20), g)
    wp = X.lattice((8, 3, 7, 7), g)
    col = F.unfold(xi, 7, padding=3, stride=4).transpose(1, 2).reshape(-1, 147)
    X.assert_exact(F.conv2d(xi.float(), wp.float(), stride=4, padding=3).permute(0, 2, 3, 1).reshape(-1, 8),
                   X.gemm_ref(0, col, wp.reshape(8, 147)), 'patch conv')
    # depthwise 7x7 + bias forward / backward, depthwise 3x3 without the GELU (backward form)
    for k in (7, 3):
        C_ = 8
        xd, wd, bd, dyd = X.lattice((Bn * H * W, C_), g), X.lattice((C_, k * k), g), X.integers((C_,), g), X.lattice((Bn * H * W, C_), g)
        xn = xd.float().reshape(Bn, H, W, C_).permute(0, 3, 1, 2).requires_grad_(True)
        wn = wd.float().reshape(C_, 1, k, k).requires_grad_(True)
        bn_ = bd.float().requires_grad_(True)
        y = F.conv2d(xn, wn, bn_, padding=k // 2, groups=C_)
        y.backward(dyd.float().reshape(Bn, H, W, C_).permute(0, 3, 1, 2))
        X.assert_exact(tok(y.detach()), X.dwconv_ref(xd, wd, bd, Bn, H, W, C_, k), f'dwconv{k} forward')
        rdx, rdw, rdb = X.dwconv_bwd_ref(xd, wd, dyd, Bn, H, W, C_, k)
        X.assert_exact(tok(xn.grad), rdx, f'dwconv{k} dx')
        X.assert_exact(wn.grad.reshape(C_, k * k), rdw, f'dwconv{k} dw')
        X.assert_exact(bn_.grad, rdb, f'dwconv{k} db')
    # bilinear by 2, 4, 8 (align_corners=False): weights are multiples of 1/16, products of 1/256
    for r in (2, 4, 8):
        h, w_, C_ = 3, 5, 8
        xs, do = X.lattice((Bn * h * w_, C_), g), X.lattice((Bn * h * r * w_ * r, C_), g)
        xn = xs.float().reshape(Bn, h, w_, C_).permute(0, 3, 1, 2).requires_grad_(True)
        y = F.interpolate(xn, size=(h * r, w_ * r), mode='bilinear', align_corners=False)
        y.backward(do.float().reshape(Bn, h * r, w_ * r, C_).permute(0, 3, 1, 2))
        X.assert_exact(tok(y.detach()), X.bilinear_ref(xs, Bn, h, w_, C_, h * r, w_ * r), f'bilinear x{r}')
        X.assert_exact(tok(xn.grad), X.bilinear_bwd_ref(do, Bn, h, w_, C_, h * r, w_ * r), f'bilinear x{r} backward')


def _attention_autograd(q, k, v, d_o, B, heads, N, Nkv, hd, scale):
    q, k, v = (t.float().requires_grad_(True) for t in (q, k, v))
    o = X.attention_fp32(q, k, v, B, heads, N, Nkv, hd, scale)
    o.backward(d_o.float())
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize('shape', [(2, 2, 300, 300, 64), (1, 3, 100, 37, 32), (2, 1, 130, 256, 32)])
def test_known_answer_attention_on_torch_fp32(shape):
    """Selector and uniform inputs: torch's fp32 softmax attention and its autograd reproduce the closed forms bit for bit (O, dQ = 0,
    dK = 0, dV; uniform: O, to one unit in the last place of bf16 where 1 / Nkv is not exact)."""
    B, heads, N, Nkv, hd = shape
    scale = hd ** -0.5
    assert X.selector_margin(Nkv, hd, scale) > 110
    q, k, v, d_o, pi = X.selector_inputs(B, heads, N, Nkv, hd, X.gen(31))
    for t in (q, k, v, d_o):
        assert torch.equal(t.to(BF).double(), t)
    assert {0, Nkv - 1} <= set(pi[0, 0].tolist()) and (Nkv <= 32 or {31, 32} <= set(pi[-1, -1].tolist()))
    want = X.selector_answers(v, d_o, pi, B, heads, N, Nkv, hd)
    for name, got, ref in zip(('O', 'dQ', 'dK', 'dV'), _attention_autograd(q, k, v, d_o, B, heads, N, Nkv, hd, scale), want):
        X.assert_exact(got, ref, f'selector {name}')
        X.assert_exact(got.to(BF), ref, f'selector {name} bf16')
    q, k, v = X.uniform_inputs(B, heads, N, Nkv, hd, X.gen(32))
    o = X.attention_fp32(q, k, v, B, heads, N, Nkv, hd, scale)
    pow2 = Nkv & (Nkv - 1) == 0
    ref = X.uniform_answer(v, B, heads, N, Nkv, hd)
    if pow2:
        X.assert_exact(o, ref, 'uniform O')
    X.assert_exact(o.to(BF), ref, 'uniform O bf16', ulp=0 if pow2 else 1)


def _mutants():
    """(name, wrong result, float64 reference, ulp): deliberately wrong computations, each of which today's 3 % bar lets through."""
    out = []
    M, N, K = 300, 150, 4608
    A, B, bias, res, rs, rpg = _gemm_problem(0, M, N, K, 40)
    ref = X.gemm_ref(0, A, B, bias, res, rs, rpg)
    good = _gemm_fp32(0, A, B, bias, res, rs, rpg)
    assert X.is_exact(good, ref) and X.is_exact(good.to(BF), ref)
    for dt in (F32, BF):
        out.append((f'last K element dropped {dt}', _gemm_fp32(0, A[:, :-1], B[:, :-1], bias, res, rs, rpg).to(dt), ref, 0))
        m = good.clone()
        m[-1] = m[-2]
        out.append((f'last row copied from its neighbour {dt}', m.to(dt), ref, 0))
        m = good.clone()
        m[:, -1] = m[:, -2]
        out.append((f'last column copied from its neighbour {dt}', m.to(dt), ref, 0))
    A0, B0 = _gemm_problem(0, M, N, K, 41, epilogue=False)[:2]
    ref0 = X.gemm_ref(0, A0, B0)
    h = K // 2
    halves = (A0[:, :h].float() @ B0[:, :h].float().t()).to(BF).float() + (A0[:, h:].float() @ B0[:, h:].float().t()).to(BF).float()
    out.append(('two K halves rounded to bf16 before the add (fp32 out)', halves, ref0, 0))
    out.append(('two K halves rounded to bf16 before the add (bf16 out)', halves.to(BF), ref0, 0))
    out.append(('output truncated instead of rounded', X.trunc_bf16(A0.float() @ B0.float().t()), ref0, 0))
    # weight gradient over 131072 pixels
    g = X.gen(42)
    Kt = 131072
    dy, x = X.lattice((Kt, 64), g), X.lattice((Kt, 96), g)
    rw, rb = X.dw_db_ref(dy, x)
    dyf, xf = dy.float(), x.float()
    full = dyf.t() @ xf
    for slab in (128, 256):
        s0 = 4096
        part = dyf[s0:s0 + slab].t() @ xf[s0:s0 + slab]
        out.append((f'one {slab}-row K slab dropped', full - part, rw, 0))
        out.append((f'one {slab}-row K slab counted twice', full + part, rw, 0))
    out.append(('last 1024 pixels never accumulated', dyf[:-1024].t() @ xf[:-1024], rw, 0))
    out.append(('last pixel missing from the bias gradient', dyf[:-1].sum(0), rb, 0))
    # conv: one border tap of one channel taken from the neighbouring pixel instead of the zero padding
    Bn, H, W, I, O = 1, 6, 6, 8, 8
    xt, wm = X.lattice((Bn * H * W, I), g), X.lattice((O, 9 * I), g)
    xp = F.pad(xt.float().reshape(Bn, H, W, I).permute(0, 3, 1, 2), (1, 1, 1, 1))
    xp[:, 0, 1:2, 0] = xp[:, 0, 1:2, 1]
    y = F.conv2d(xp, wm.float().reshape(O, 3, 3, I).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(Bn * H * W, O)
    out.append(('one border tap of one channel from the neighbouring pixel', y, X.conv3x3_ref(0, xt, wm, Bn, H, W, I, O), 0))
    out.append(('the same, bf16 out', y.to(BF), X.conv3x3_ref(0, xt, wm, Bn, H, W, I, O), 0))
    # attention
    B_, heads, Nq, Nkv, hd = 1, 2, 200, 256, 32
    scale = hd ** -0.5
    q, k, v, d_o, pi = X.selector_inputs(B_, heads, Nq, Nkv, hd, X.gen(43))
    o, dq, dk, dv = X.selector_answers(v, d_o, pi, B_, heads, Nq, Nkv, hd)
    drop = lambda t, rows: torch.cat([t.reshape(B_, Nkv, -1)[:, :rows[0]], t.reshape(B_, Nkv, -1)[:, rows[1]:]], 1).reshape(-1, heads * hd)   # noqa: E731
    for name, rows in (('one key skipped', (32, 33)), ('the last key tile skipped', (Nkv - 32, Nkv))):
        n2 = Nkv - (rows[1] - rows[0])
        out.append((f'selector: {name}', X.attention_fp32(q, drop(k, rows), drop(v, rows), B_, heads, Nq, n2, hd, scale).to(BF), o, 0))
    wrong = X.selector_answers(v, d_o, pi.roll(1, dims=1), B_, heads, Nq, Nkv, hd)
    out.append(('selector: pi of the wrong head (O)', wrong[0].to(BF), o, 0))
    out.append(('selector: pi of the wrong head (dV)', wrong[3].to(BF), dv, 0))
    for nkv in (256, 37):
        qu, ku, vu = X.uniform_inputs(B_, heads, Nq, nkv, hd, X.gen(44))
        refu = X.uniform_answer(vu, B_, heads, Nq, nkv, hd)
        ulp = 0 if nkv == 256 else 1
        assert X.is_exact(X.attention_fp32(qu, ku, vu, B_, heads, Nq, nkv, hd, scale).to(BF), refu, ulp)
        dropu = lambda t: t.reshape(B_, nkv, -1)[:, :-1].reshape(-1, heads * hd)          # noqa: E731
        out.append((f'uniform, {nkv} keys: one key skipped',
                    X.attention_fp32(qu, dropu(ku), dropu(vu), B_, heads, Nq, nkv - 1, hd, scale).to(BF), refu, ulp))
        twice = torch.cat([vu.reshape(B_, nkv, -1), vu.reshape(B_, nkv, -1)[:, :1]], 1).sum(1) / nkv
        out.append((f'uniform, {nkv} keys: one key counted twice',
                    twice[:, None].expand(B_, Nq, heads * hd).reshape(-1, heads * hd).float().to(BF), refu, ulp))
    return out


def test_every_mutant_fails_the_comparison_the_gpu_tests_use():
    """The tests have teeth: each deliberately wrong computation is rejected by X.mismatch_report (through is_exact), and the report names
    the count, the first elements and the pattern of the wrong ones."""
    muts = _mutants()
    assert len(muts) >= 25
    passed = [name for name, got, ref, ulp in muts if X.is_exact(got, ref, ulp)]
    assert not passed, passed
    name, got, ref, ulp = next(m for m in muts if m[0].startswith('last column copied'))
    msg = X.mismatch_report(got, X.expected(ref, got.dtype), name)
    assert 'all in column 149' in msg and 'elements wrong' in msg and '(row ' in msg, msg
    name, got, ref, ulp = next(m for m in muts if m[0].startswith('last row copied'))
    assert 'all in row 299' in X.mismatch_report(got, X.expected(ref, got.dtype), name)
    # a fault with a period shows as a residue: every 16th column wrong
    ref = X.lattice((64, 64), X.gen(45))
    bad = ref.float().clone()
    bad[:, 5::16] += 1
    assert 'column mod 16 in [5]' in X.mismatch_report(bad, ref.float(), 'periodic')


def test_round_bf16_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2 ** -8 + 2 ** -30, 257.0, 259.0, -3.0, 0.0, 1 / 3], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.015625, 1.0078125, 256.0, 260.0, -3.0, 0.0, 0.333984375], dtype=torch.float64)
    assert torch.equal(X.round_bf16(x).double(), want)
    # float64 -> fp32 -> bf16 would round 1 + 2^-8 + 2^-30 down to 1 + 2^-8 first and then, on the tie, to even (1.0): one rounding does not
    assert x[3].float().to(BF).item() == 1.0 and X.round_bf16(x[3:4]).item() == 1.0078125


# =================================================== GPU ==============================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_exact_table_row(case):
    """One row of the dispatch table, reduced, and its ragged neighbours: exact outputs, nothing written outside them, and the trace names
    the row's kernels (every (entry point, kernel) pair of EXACT_PAIRS is in one of these assertions)."""
    cfg, e = CASES[case]
    r = reduce_case(e)
    for c in [r] + ragged_neighbours(r):
        ran = run_case(c)
        assert _same_kernels(e, ran), (c['args'], ran, e['kernels'])


SWITCHES = [('SEGFAC_GEMM_NO_TR', '1', ('segf_gemm', 'segf_gemm_dw_db')), ('SEGFAC_GEMM_NO_BIG', '1', ('segf_gemm', 'segf_gemm_dw_db')),
            ('SEGFAC_GEMM8_DW', '0', ('segf_gemm_dw_db_grouped',)), ('SEGFAC_ATTN64_DKV_ROWS', '32', ('segf_attention_bwd',)),
            ('SEGFAC_ATTN64_DKV_ROWS', '64', ('segf_attention_bwd',)), ('SEGFAC_ATTN64_PRESCALE', '1', ('segf_attention_fwd', 'segf_attention_bwd')),
            ('SEGFAC_ATTN_NO_FUSED_BWD', '1', ('segf_attention_bwd',))]


@pytest.mark.gpu
@pytest.mark.parametrize('env,value,fns', SWITCHES, ids=['%s=%s' % s[:2] for s in SWITCHES])
def test_exact_under_policy_switch(env, value, fns, monkeypatch):
    """The forms reachable only through a policy switch: the cases of the named entry points whose dry-run kernel names the switch changes
    (the tile-row and prescale switches select other template arguments of the head-dim-64 kernels and leave the head-dim-32 cases alone),
    with the same exact answers.  SEGFAC_ATTN64_PRESCALE rounds q * scale * log2(e) to bf16 once more: the selector margin moves by that one
    rounding (2^-9 relative, still > 100) and a zero query stays zero, so the forward, dQ and dK stay exact; selector dV does not
    (derivation in run_attention) and the uniform dV takes its place."""
    from segmentation_factory_amd import hip
    reduced = [reduce_case(e) for _, e in CASES if e['fn'] in fns]                 # reduced under the default policy
    default = [_dry(r) for r in reduced]
    monkeypatch.setenv(env, value)
    assert hip.policy(env) == int(value)
    ran = 0
    for r, was in zip(reduced, default):
        want = _dry(r)
        assert want, (env, r['args'], 'the entry point refuses the case under the switch')
        if want == was:
            continue
        got = run_case(r)
        assert got == want, (r['args'], got, want)
        ran += 1
    assert ran >= 1, 'the switch changed no case'


def _first_case(fn, pred=lambda e: True):
    return next(reduce_case(e) for _, e in CASES if e['fn'] == fn and pred(e))


@pytest.mark.gpu
@pytest.mark.parametrize('split', [1, 2, 3, 'pick'])
def test_exact_weight_gradient_split_counts(split):
    """Explicit split-K counts 1, 2, 3 and the picker's own choice, through segf_gemm (layout 2), segf_gemm_dw_db and the conv weight gradient."""
    from segmentation_factory_amd import hip
    r = _first_case('segf_gemm', lambda e: e['args'][1] == 2)
    M, N, K = r['args'][2:5]
    s = hip.pick_splitk(M, N, K) if split == 'pick' else split
    c = _with(r, split_k=s, ws='p0' if s > 1 else None)
    assert run_case(c) == _dry(c) != []
    r = _first_case('segf_gemm_dw_db')
    M, N, K = r['args'][1:4]
    c = _with(r, split_k=hip.pick_splitk(M, N, K) if split == 'pick' else split)
    assert run_case(c) == _dry(c) != []
    r = _first_case('segf_conv3x3', lambda e: e['args'][0] == 2)
    _, Bc, Hc, Wc, Cin, Cout = r['args'][:6]
    s = hip.pick_splitk_conv3x3(Cin, Cout, Bc * Hc * Wc) if split == 'pick' else split
    c = _with(r, split_k=s, ws='p0' if s > 1 else None)
    assert run_case(c) == _dry(c) != []


# ---- beside the table: ragged feature sizes, and the spatial kernels ------------------------------------------------------------------
def _gemm_entry(layout, M, N, K, c_dt, epilogue, split_k=1):
    """A segf_gemm call outside the table: dense operands (leading dimension = width, so odd widths are unaligned rows)."""
    (ar, ac), (br, bc) = X.gemm_operand_shapes(layout, M, N, K)
    ep = ['p0', 'p0', N, 'p0', 100] if epilogue else [None, None, 0, None, 1]
    return {'fn': 'segf_gemm', 'kernels': [],
            'args': [1, layout, M, N, K, 'p0', ac, 'p0', bc, 'p0', c_dt, N] + ep + [split_k, 'p0' if split_k > 1 else None, None]}


RAGGED_FEATURES = [(lay, M, N, K) for lay in (0, 1) for M, N, K in ((1000, 129, 255), (1000, 127, 257), (300, 255, 129), (513, 257, 127), (2049, 33, 31))] \
    + [(2, M, N, K) for M, N, K in ((129, 255, 4097), (127, 257, 4095), (257, 127, 1031), (33, 31, 70001))]


@pytest.mark.gpu
@pytest.mark.parametrize('layout,M,N,K', RAGGED_FEATURES)
def test_exact_feature_ragged_gemm(layout, M, N, K):
    """M, N and K one more and one less than multiples of 32 / 128 / 256 (the table's feature sizes are all tile multiples): bf16 out with
    bias, residual and row scale (layouts 0, 1), fp32 out with 1 and 3 K slices (layout 2).  The kernels are whatever the dispatch takes;
    the trace must name some and agree with the dry run."""
    cases = [_gemm_entry(layout, M, N, K, 1, True), _gemm_entry(layout, M, N, K, 1, False)] if layout != 2 else \
        [_gemm_entry(2, M, N, K, 0, False, 1), _gemm_entry(2, M, N, K, 0, False, 3)]
    for c in cases:
        want = _dry(c)
        assert want, c['args']
        assert run_case(c) == want


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [BF, F32], ids=['bf16', 'fp32'])
def test_exact_spatial_kernels(dtype):
    """Depthwise 7 x 7 + bias forward / backward, depthwise 3 x 3 backward without the GELU, bilinear resize by 2 / 4 / 8 and the column sum
    on lattice inputs with integer bias, odd image sizes (every border on all four sides) and two images: exact as the matrix kernels are."""
    from segmentation_factory_amd import hip
    g = X.gen(70)
    dev = lambda t, dt=dtype: t.to(dt).cuda().contiguous()                                # noqa: E731
    B, H, W, C_ = 2, 13, 9, 24
    P = B * H * W
    x64, dy64, b64 = X.lattice((P, C_), g), X.lattice((P, C_), g), X.integers((C_,), g)
    for k in (7, 3):
        w64 = X.lattice((C_, k * k), g)
        rdx, rdw, rdb = X.dwconv_bwd_ref(x64, w64, dy64, B, H, W, C_, k)
        with hip.trace() as t:
            if k == 7:
                wt = dev(w64.t(), F32)
                y = hip.dwconv7x7_fwd(dev(x64), wt, dev(b64, F32), B, H, W, C_)
                dx, dw, db = hip.dwconv7x7_bwd(dev(x64), wt, dev(dy64), B, H, W, C_)
            else:
                y = None
                dx, dw, db = hip.dwconv3x3_gelu_bwd(dev(x64), dev(w64, F32), dev(b64, F32), dev(dy64), B, H, W, C_, apply_gelu=False)
        torch.cuda.synchronize()
        assert t.kernels
        if y is not None:
            X.assert_exact(y, X.dwconv_ref(x64, w64, b64, B, H, W, C_, k), f'dwconv{k} forward')
        X.assert_exact(dx, rdx, f'dwconv{k} dx')
        X.assert_exact(dw, rdw, f'dwconv{k} dw')
        X.assert_exact(db, rdb, f'dwconv{k} db')
    for r in (2, 4, 8):
        h, w_ = 5, 7
        xs64 = X.lattice((B * h * w_, C_), g)
        out = torch.empty(B * h * r * w_ * r, C_, dtype=dtype, device='cuda')
        with hip.trace() as t:
            hip.bilinear_fwd(dev(xs64), B, h, w_, C_, h * r, w_ * r, out)
        torch.cuda.synchronize()
        assert t.kernels
        X.assert_exact(out, X.bilinear_ref(xs64, B, h, w_, C_, h * r, w_ * r), f'bilinear x{r}')
    rows64 = X.lattice((70001, 40), g)
    X.assert_exact(hip.colsum(dev(rows64)), rows64.sum(0), 'colsum')


def _depthwise_form_params():
    """Every 3 x 3 shape of tests/dwconv_refs.py less (2, 32, 32, 64), both dtypes, every form that admits the shape."""
    import dwconv_refs as D
    out = []
    for shape, _ in D.SHAPES3:
        if shape == (2, 32, 32, 64):
            continue
        for dt, name in ((BF, 'bf16'), (F32, 'fp32')):
            for form, rows in D.forms3(dict(shape=shape), dt, True):
                out.append(pytest.param(shape, dt, form, rows, id=f'{"x".join(map(str, shape))}-{name}-{form}{f"-rows{rows}" if rows else ""}'))
    return out


def _lattice_rows(shape, g):
    """Lattice activations as the float64 [B][H][W][C] map of the references and as their [rows][C] view."""
    t = X.lattice(shape, g)
    return t, t.reshape(-1, shape[-1])


@pytest.mark.gpu
@pytest.mark.parametrize('shape,dtype,form,rows', _depthwise_form_params())
def test_exact_depthwise_forms(shape, dtype, form, rows, monkeypatch):
    """The depthwise 3 x 3 WITHOUT the GELU on lattice inputs with integer bias, zero tolerance, in every form of csrc/conv.hip (strip,
    vertical walk with its row switch, one-launch) at the shapes where the dispatch changes (tests/dwconv_refs.py SHAPES3): the forward
    (strip and walk; the one-launch form has none) and dx, dw, db of the backward.  The form is forced with the existing switches and
    asserted with hip.trace().  The references are the float64 slice sums of dwconv_refs: sums of small integers, exact in any order."""
    import dwconv_refs as D
    from segmentation_factory_amd import hip
    B, H, W, C_ = shape
    assert B * H * W < X.FP32_EXACT_TERMS                      # every dw / db sum stays exact in fp32
    g = X.gen(71)
    dev = lambda t, dt=dtype: t.to(dt).cuda().contiguous()                                # noqa: E731
    (x4, x2), (dy4, dy2) = _lattice_rows(shape, g), _lattice_rows(shape, g)
    w64, b64 = X.lattice((C_, 9), g), X.integers((C_,), g)
    D.force_form(monkeypatch, form, rows)
    if form != 'small':
        with hip.trace() as t:
            y = hip.dwconv3x3_gelu_fwd(dev(x2), dev(w64, F32), dev(b64, F32), B, H, W, C_, apply_gelu=False)
        torch.cuda.synchronize()
        D.assert_form_ran(t, form, dtype, False)
        X.assert_exact(y, D.fwd_ref(x4, w64, b64, 3, False)['y'], f'dwconv3 {form} forward')
    with hip.trace() as t:
        dx, dw, db = hip.dwconv3x3_gelu_bwd(dev(x2), dev(w64, F32), dev(b64, F32), dev(dy2), B, H, W, C_, apply_gelu=False)
    torch.cuda.synchronize()
    D.assert_form_ran(t, form, dtype, True)
    rdw, rdb, _, _ = D.wgrad_ref(x4, dy4, 3)
    X.assert_exact(dx, D.dx_ref(dy4, w64, 3)[0], f'dwconv3 {form} dx')
    X.assert_exact(dw, rdw, f'dwconv3 {form} dw')
    X.assert_exact(db, rdb, f'dwconv3 {form} db')


def _depthwise7_params():
    import dwconv_refs as D
    return [pytest.param(s, dt, id=f'{"x".join(map(str, s))}-{name}') for s, _ in D.SHAPES7 for dt, name in ((BF, 'bf16'), (F32, 'fp32'))]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,dtype', _depthwise7_params())
def test_exact_depthwise7_shapes(shape, dtype):
    """The depthwise 7 x 7 forward (+ integer bias) and backward on lattice inputs at the shapes of tests/dwconv_refs.py SHAPES7: one pixel, a
    map smaller than the kernel, strips whose last has one live pixel, two channel slabs in the weight gradient."""
    import dwconv_refs as D
    from segmentation_factory_amd import hip
    B, H, W, C_ = shape
    assert B * H * W < X.FP32_EXACT_TERMS
    g = X.gen(72)
    dev = lambda t, dt=dtype: t.to(dt).cuda().contiguous()                                # noqa: E731
    (x4, x2), (dy4, dy2) = _lattice_rows(shape, g), _lattice_rows(shape, g)
    w64, b64 = X.lattice((C_, 49), g), X.integers((C_,), g)
    wt = dev(w64.t(), F32)
    with hip.trace() as t:
        y = hip.dwconv7x7_fwd(dev(x2), wt, dev(b64, F32), B, H, W, C_)
        dx, dw, db = hip.dwconv7x7_bwd(dev(x2), wt, dev(dy2), B, H, W, C_)
    torch.cuda.synchronize()
    for n in ('dwconv7x7_kernel<T, false>', 'dwconv7x7_kernel<T, true>', 'dwconv7x7_wgrad_kernel<T>', 'dw7_scatter_kernel'):
        assert any(n in k for k in t.kernels), (n, t.kernels)
    rdw, rdb, _, _ = D.wgrad_ref(x4, dy4, 7)
    X.assert_exact(y, D.fwd_ref(x4, w64, b64, 7, False)['y'], 'dwconv7 forward')
    X.assert_exact(dx, D.dx_ref(dy4, w64, 7)[0], 'dwconv7 dx')
    X.assert_exact(dw, rdw, 'dwconv7 dw')
    X.assert_exact(db, rdb, 'dwconv7 db')


@pytest.mark.gpu
def test_exact_depthwise7_second_strip_of_a_thread():
    """dwconv7x7_kernel runs more than one strip per thread only from about 67 M elements on (dw7_blocks: units * (C / 8) / 256 / 2048 >= 2),
    which every ConvNeXt stage of the benchmark reaches and no other test does.  (8, 128, 128, 512) in bf16 on lattice inputs, forward
    (+ integer bias) and dx: 2 strips per thread, asserted with the host arithmetic restated here.  Compared exactly on a sample -- 8192
    pixels drawn with a fixed seed, the four corners and one full border row and column of the first and last image, all channels -- whose
    float64 reference is gathered on the CPU for those pixels only, so the case costs no full-size float64 convolution.  The weight
    gradient is left out at this size: it has no sampled form (every one of its 49 x 512 sums runs over all 131072 pixels, a full-size
    reference), and its plan is covered by the small shapes of test_exact_depthwise7_shapes."""
    import dwconv_refs as D
    from segmentation_factory_amd import hip
    B, H, W, C_ = 8, 128, 128, 512
    units = B * H * ((W + 7) // 8)
    assert min(4, max(1, units * (C_ // 8) // 256 // 2048)) == 2 == D.dw7_strips_per_thread(B, H, W, C_)
    g = X.gen(73)
    x8, dy8 = D.lattice_i8((B, H, W, C_), g), D.lattice_i8((B, H, W, C_), g)
    w64, b64 = X.lattice((C_, 49), g), X.integers((C_,), g)
    pix = D.sample_pixels(B, H, W, 8192, g)
    rows = (pix[:, 0] * H + pix[:, 1]) * W + pix[:, 2]
    wt = w64.t().float().cuda().contiguous()
    xd, dyd = x8.reshape(-1, C_).to(BF).cuda(), dy8.reshape(-1, C_).to(BF).cuda()
    with hip.trace() as t:
        y = hip.dwconv7x7_fwd(xd, wt, b64.float().cuda(), B, H, W, C_)
        dx, _, _ = hip.dwconv7x7_bwd(xd, wt, dyd, B, H, W, C_)
    torch.cuda.synchronize()
    assert any('dwconv7x7_kernel<T, false>' in k for k in t.kernels) and any('dwconv7x7_kernel<T, true>' in k for k in t.kernels), t.kernels
    ys, dxs = y[rows.cuda()].cpu(), dx[rows.cuda()].cpu()
    X.assert_exact(ys, D.gathered_conv7(x8, w64, b64, pix, 1), 'dwconv7 forward, second strip of a thread')
    X.assert_exact(dxs, D.gathered_conv7(dy8, w64, None, pix, -1), 'dwconv7 dx, second strip of a thread')


NEIGHBOURS = [0, 1, 4, 0, 2, 3, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 4, 4, 2, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 2, 0, 2, 1, 1, 1, 1, 2, 1,
              1, 1, 1, 0, 2, 4, 2, 1, 3, 3, 0, 2, 1, 2, 0]


def test_ragged_neighbour_counts():
    """How many ragged neighbours each case runs beside its own shape (dry runs): pinned, so that a dispatch edit that takes a neighbour
    away shows.  The cases without one are the weight gradients whose kernels need whole 32-token groups or a slice count tied to the token
    count (grouped streaming kernels, 85-slice eight-phase products) and the conv weight gradient of one row; the ragged K of those forms is
    covered by test_exact_feature_ragged_gemm and test_exact_weight_gradient_split_counts.  Every entry point has cases with neighbours."""
    got = [len(ragged_neighbours(reduce_case(e))) for _, e in CASES]
    assert got == NEIGHBOURS, got
    for fn in FNS:
        assert any(n for n, (_, e) in zip(got, CASES) if e['fn'] == fn), fn
