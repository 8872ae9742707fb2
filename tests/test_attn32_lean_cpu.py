"""The scalar chain of the head-dim-32 attention backward (csrc/attention_mfma.hip, default policy) behind the forward's log-sum-exp,
restated in numpy float32 and run on the known-answer inputs of tests/exact_inputs.py, without a GPU: the exact tests
(tests/test_exact_kernels.py) need P of the chosen key to round to exactly 1.0 in bf16, P of every other key to be exactly 0 and, for the
uniform family, bf16(P) = 1 / Nkv.

The chain, as the kernels compute it:
  forward (online softmax, natural units):  m = max_j S scale;  p = exp(S scale - m);  l = sum_j p;  lse = m + log(l)
  backward:  cs = scale * log2(e) (fp32, formed once);  nl = lse * -log2(e);  p = exp2(fma(S, cs, nl))
At the selector score of head dim 32 (3200 * scale = 566, 816 in log2 units) the roundings of lse, of nl and of cs add up to at most a
few 1e-4 in the exponent (measured here: 5e-6); bf16 rounds to 1.0 within -2^-9 .. +2^-8.
"""
import json
import os

import numpy as np
import pytest

import exact_inputs as X

F = np.float32
LOG2E = F(1.44269504088896340736)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _rows():
    with open(os.path.join(GOLDEN, 'dispatch_table.json')) as fh:
        table = json.load(fh)
    seen, out = set(), []
    for cfg in sorted(table):
        for e in table[cfg]:
            a = e['args']
            if e['fn'] in ('segf_attention_fwd', 'segf_attention_bwd') and a[5] == 32:
                key = (e['fn'], a[2], a[3], a[4], a[12])
                if key not in seen:
                    seen.add(key)
                    out.append((e['fn'], a[2], a[3], a[4], a[12]))
    return out


ROWS = _rows()


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, and so is the sum at these magnitudes; one rounding."""
    return (np.asarray(a, np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(F)


def bf16(x):
    """fp32 -> bf16 (nearest even), returned as fp32."""
    u = np.asarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F)


def forward_chain(S, scale):
    """S [N][Nkv] raw scores (fp32) -> (p [N][Nkv], l [N], lse [N]): the forward's arithmetic (one multiply per score, natural exp)."""
    sc = (S * F(scale)).astype(F)
    m = sc.max(1)
    p = np.exp((sc - m[:, None]).astype(F)).astype(F)
    l = np.zeros(S.shape[0], F)
    for j in range(S.shape[1]):                      # fp32 partial sums (the order moves the sum by 1e-7 relative: immaterial here)
        l = (l + p[:, j]).astype(F)
    lse = (m + np.log(l).astype(F)).astype(F)
    return p, l, lse


def backward_p(S, scale, lse):
    cs = F(F(scale) * LOG2E)
    nl = (lse * F(-1.44269504088896340736)).astype(F)
    return np.exp2(fma32(S, cs, nl[:, None])).astype(F)


def test_the_table_has_head_dim_32_rows():
    assert {r[0] for r in ROWS} == {'segf_attention_fwd', 'segf_attention_bwd'} and len(ROWS) >= 8
    assert all(Nkv <= 256 for _, _, _, Nkv, _ in ROWS)          # every row takes the LDS-resident forward and the one-kernel backward


@pytest.mark.parametrize('row', ROWS, ids=['%s-h%d-N%d-k%d' % r[:4] for r in ROWS])
def test_selector_chain(row):
    fn, heads, N, Nkv, scale = row
    hd = 32
    g = X.gen(6)
    n = min(N, 2 * Nkv + 64)
    q, k, v, d_o, pi = X.selector_inputs(1, 1, n, Nkv, hd, g)
    S = (q.numpy() @ k.numpy().T).astype(F)                      # integers below 2^24: exact, as in the matrix pipe
    assert abs(float(S.max()) * scale * 1.4426950408889634) < 2 ** 10
    chosen = pi.reshape(-1).numpy()
    rows = np.arange(n)
    p, l, lse = forward_chain(S, scale)
    others = np.ones_like(p, dtype=bool)
    others[rows, chosen] = False
    assert (bf16(p[rows, chosen]) == 1).all(), np.abs(p[rows, chosen] - 1).max()
    assert (p[others] == 0).all()
    # O = (V^T bf16(P)) / l: exactly V[pi] once rounded to bf16
    o = ((v.numpy().astype(F)[chosen] * bf16(p[rows, chosen])[:, None]).astype(F) * (F(1) / l)[:, None]).astype(F)
    assert (bf16(o) == v.numpy().astype(F)[chosen]).all()
    pb = backward_p(S, scale, lse)
    assert (bf16(pb[rows, chosen]) == 1).all(), np.abs(pb[rows, chosen] - 1).max()
    assert (pb[others] == 0).all()
    # margin: the exponent's error is several times below bf16's half-spacing under 1 (2^-9)
    assert np.abs(pb[rows, chosen] - 1).max() < 2.0 ** -9 / 4


@pytest.mark.parametrize('row', ROWS, ids=['%s-h%d-N%d-k%d' % r[:4] for r in ROWS])
def test_uniform_chain(row):
    fn, heads, N, Nkv, scale = row
    S = np.zeros((4, Nkv), F)                                    # q = 0: every score is 0
    p, l, lse = forward_chain(S, scale)
    assert (p == 1).all() and (l == Nkv).all()
    pb = backward_p(S, scale, lse)
    want = X.round_bf16(np.float64(1.0) / X.torch.tensor([float(Nkv)], dtype=X.torch.float64)).float().numpy()[0]
    assert (bf16(pb) == want).all(), (pb.min(), pb.max())
    if Nkv & (Nkv - 1) == 0:
        assert want == 1.0 / Nkv


def test_rows_beyond_a_chunk_add_nothing():
    """The staged lse of a row beyond the query chunk is +inf: nl = -inf and p = exp2(-inf) = 0 for any finite score."""
    S = np.array([[0.0, 3200.0, -3200.0]], F)
    with np.errstate(over='ignore'):
        pb = backward_p(S, 32 ** -0.5, np.array([np.inf], F))
    assert (pb == 0).all()
