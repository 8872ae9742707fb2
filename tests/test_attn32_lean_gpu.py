"""Head-dim-32 attention with at most 256 keys under the default policy (csrc/attention_mfma.hip: attn_mfma_fwd_kernel<32, ...> and the
fma + exp2 one-kernel backward), bf16, through functional.attention, against float64 softmax attention on the CPU from the bf16-rounded
inputs.

Shapes (B, heads, N, Nkv) and what each one can break:
  (2, 1, 200, 256)   all eight 32-key steps, N not a multiple of the 128-query workgroup
  (1, 2, 70, 200)    masked last step, partial query tile
  (2, 5, 64, 37)     two steps, the second masked, five heads for the row strides
  (1, 8, 16, 4)      a single masked step, fewer queries than one tile
  (1, 1, 33, 64)     a lone row in the second query tile
  (3, 2, 1000, 256)  more than one query chunk in the backward

Tolerances are those of tests/test_kernels_gpu.py::test_attention (3 % of the tensor's largest magnitude + 3e-4, times 1 / 2 / 4 for
O / dQ / d[k | v]).  lse: 1e-3 absolute or 1e-5 relative (fp32 storage of a value of up to a few hundred; the kernel's log2 / exp2 are
accurate to one unit in the last place)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HD = 32
SHAPES = [(2, 1, 200, 256), (1, 2, 70, 200), (2, 5, 64, 37), (1, 8, 16, 4), (1, 1, 33, 64), (3, 2, 1000, 256)]
IDS = ['%dx%dx%dx%d' % s for s in SHAPES]
FWD, BWD, REDUCE = 'attn_mfma_fwd_kernel<32, QW, false, 4, false>', 'attn_mfma_bwd_fused_kernel<32, 4>', 'attn_dkv_reduce_kernel<bf16_t>'


def _tol(ref, fac):
    return fac * (3e-2 * ref.abs().max().item() + 3e-2 * 1e-2)          # test_kernels_gpu._close for bf16


def _heads(t, B, n, heads):
    return t.reshape(B, n, heads, HD).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def problem(shape, family):
    """bf16-rounded inputs (CPU, as float64) and the float64 oracle: (q, kv, do, o, lse, dq, dkv).  Computed once per (shape, family)."""
    B, heads, N, Nkv = shape
    C = heads * HD
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B * N, C, generator=g)
    kv = torch.randn(B * Nkv, 2 * C, generator=g)
    do = torch.randn(B * N, C, generator=g)
    if family != 'normal':
        # Peaky rows whose scores ascend (or descend) with the key index for EVERY query.  The head's 32 dims are split three ways:
        #   dims  0..15  the ordering direction: k_j = tau_j s with s a sign vector and tau_j monotone, q flipped so that q . s > 0;
        #   dims 16..23  q only (k = 0);   dims 24..31  k only (q = 0): neither moves a score, so every row stays monotone.
        # Both at 6 times the unit scale of the normal family (tau: rms 6.9).  The k-only dims are what keeps dQ = dS K well conditioned:
        # with rank-one keys alone, dQ = s sum_j dS_ij tau_j is a cancelling sum (sum_j dS_ij = 0) whose largest element is far below
        # the bf16 rounding of the dS operand times |tau| <= 12, whatever arithmetic forms P -- a bound relative to max |dQ| then
        # measures that conditioning and not the kernel.
        s = (torch.randint(0, 2, (heads, 16), generator=g) * 2 - 1).float()
        tau = 24.0 * (torch.arange(Nkv).float() - (Nkv - 1) / 2) / Nkv
        if family == 'descending':
            tau = tau.flip(0)
        k4 = (6 * kv[:, :C]).reshape(B, Nkv, heads, HD).clone()
        k4[..., :16] = (tau[None, :, None, None] * s[None, None]).expand(B, Nkv, heads, 16)
        k4[..., 16:24] = 0
        kv[:, :C] = k4.reshape(B * Nkv, C)
        q4 = (6 * q).to(BF).float().reshape(B * N, heads, HD)          # (rounded first: the flip below is exact in bf16)
        q4[..., 24:] = 0
        proj = (q4[..., :16].double() * s[None]).sum(-1, keepdim=True)
        q4[..., :16] = q4[..., :16] * torch.where(proj < 0, -1.0, 1.0)
        q = q4.reshape(B * N, C)
    q, kv, do = (t.to(BF).double() for t in (q, kv, do))
    qr, kvr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    k, v = kvr[:, :C], kvr[:, C:]
    sc = (_heads(qr, B, N, heads) @ _heads(k, B, Nkv, heads).transpose(-1, -2)) * HD ** -0.5           # [B][heads][N][Nkv]
    o = (sc.softmax(-1) @ _heads(v, B, Nkv, heads)).permute(0, 2, 1, 3).reshape(B * N, C)
    o.backward(do)
    lse = torch.logsumexp(sc.detach(), -1)
    out = dict(q=q, kv=kv, do=do, o=o.detach(), lse=lse, dq=qr.grad, dkv=kvr.grad, scores=sc.detach())
    assert all(torch.isfinite(t).all() for t in out.values())
    assert (sc.detach().abs() * 1.4426950408889634).max().item() < 2 ** 10          # inside the exponent range of exp2 in fp32
    if family != 'normal':
        d = sc.detach()[..., 1:] - sc.detach()[..., :-1]
        assert (d > 0).all() if family == 'ascending' else (d < 0).all()
    return out


def run(p, shape):
    """(o, dq, dkv) of functional.attention on the device, as CPU tensors in bf16."""
    from segmentation_factory_amd import functional as Fh
    B, heads, N, Nkv = shape
    qd, kvd = p['q'].to(BF).cuda().requires_grad_(True), p['kv'].to(BF).cuda().requires_grad_(True)
    o = Fh.attention(qd, kvd, B, N, Nkv, heads)
    o.backward(p['do'].to(BF).cuda())
    torch.cuda.synchronize()
    return o.detach().cpu(), qd.grad.cpu(), kvd.grad.cpu()


def errors(got, p, C):
    """Largest absolute error of O, dQ, dK, dV against the oracle."""
    o, dq, dkv = (t.double() for t in got)
    return {'O': (o - p['o']).abs().max().item(), 'dQ': (dq - p['dq']).abs().max().item(),
            'dK': (dkv[:, :C] - p['dkv'][:, :C]).abs().max().item(), 'dV': (dkv[:, C:] - p['dkv'][:, C:]).abs().max().item()}


def check_parity(got, p):
    o, dq, dkv = (t.double() for t in got)
    for name, a, ref, fac in (('O', o, p['o'], 1), ('dQ', dq, p['dq'], 2), ('dKV', dkv, p['dkv'], 4)):
        err = (a - ref).abs().max().item()
        print(f'{name}: max err {err:.3e}, bound {_tol(ref, fac):.3e}')
        assert err <= _tol(ref, fac), (name, err, _tol(ref, fac))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_oracle_parity_and_bit_reproducibility(shape):
    """Unit-normal inputs: O, dQ, d[k | v] within test_attention's tolerances of the float64 oracle; a second run of forward + backward
    returns the same bits."""
    p = problem(shape, 'normal')
    first = run(p, shape)
    check_parity(first, p)
    again = run(p, shape)
    for name, a, b in zip(('o', 'dq', 'dkv'), first, again):
        assert torch.equal(a, b), (name, (a != b).sum().item())


@pytest.mark.parametrize('family', ['ascending', 'descending'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_hard_softmax_rows(shape, family):
    """Peaky rows (q and k at 6 times the unit scale) whose scores ascend with the key index -- every step raises a running maximum --
    or descend: same tolerances, and lse against the float64 value."""
    from segmentation_factory_amd import hip
    B, heads, N, Nkv = shape
    C = heads * HD
    p = problem(shape, family)
    check_parity(run(p, shape), p)
    qd, kvd = p['q'].to(BF).cuda(), p['kv'].to(BF).cuda()
    o, lse = hip.attention_fwd(qd, kvd[:, :C], kvd[:, C:], B, heads, N, Nkv, HD, HD ** -0.5)
    torch.cuda.synchronize()
    err = (lse.double().cpu() - p['lse']).abs()
    bound = torch.maximum(torch.full_like(err, 1e-3), 1e-5 * p['lse'].abs())
    print(f'lse: max err {err.max().item():.3e} at |lse| up to {p["lse"].abs().max().item():.1f}')
    assert (err <= bound).all(), (err.max().item(), p['lse'].abs().max().item())


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_no_worse_than_the_classic_arithmetic(shape, monkeypatch):
    """Same inputs, same process: the error of O, dQ, dK, dV against the float64 oracle under the default policy is no larger than under
    SEGFAC_ATTN32_CLASSIC=1 by more than one bf16 unit in the last place of that tensor's largest magnitude."""
    from segmentation_factory_amd import hip
    C = shape[1] * HD
    p = problem(shape, 'normal')
    assert hip.policy('attn32_classic') == 0
    new = errors(run(p, shape), p, C)
    monkeypatch.setenv('SEGFAC_ATTN32_CLASSIC', '1')
    assert hip.policy('attn32_classic') == 1
    classic = errors(run(p, shape), p, C)
    big = {'O': p['o'], 'dQ': p['dq'], 'dK': p['dkv'][:, :C], 'dV': p['dkv'][:, C:]}
    for name in ('O', 'dQ', 'dK', 'dV'):
        m = big[name].abs().max().item()
        ulp = 2.0 ** (torch.tensor(m).log2().floor().item() - 7)
        print(f'{name}: new {new[name]:.4e} classic {classic[name]:.4e} ratio {new[name] / max(classic[name], 1e-30):.3f} (ulp {ulp:.2e})')
        assert new[name] <= classic[name] + ulp, (name, new[name], classic[name], ulp)


def test_the_default_policy_launches_the_table_spellings(monkeypatch):
    """(2, 1, 4096, 256, 32): the default policy runs the new backward under the spelling of tests/golden/dispatch_table.json; the classic
    switch launches a differently spelled instantiation of it (the forward has one form)."""
    from segmentation_factory_amd import hip
    B, heads, N, Nkv = 2, 1, 4096, 256
    C = heads * HD
    g = torch.Generator().manual_seed(3)
    q, do = (torch.randn(B * N, C, generator=g).to(BF).cuda() for _ in range(2))
    kv = torch.randn(B * Nkv, 2 * C, generator=g).to(BF).cuda()

    def names():
        dkv = torch.empty_like(kv)
        with hip.trace() as t:
            o, lse = hip.attention_fwd(q, kv[:, :C], kv[:, C:], B, heads, N, Nkv, HD, HD ** -0.5)
            hip.attention_bwd(q, kv[:, :C], kv[:, C:], o, do, lse, B, heads, N, Nkv, HD, HD ** -0.5, dkv[:, :C], dkv[:, C:])
        torch.cuda.synchronize()
        return [k.split(' [')[0].strip('()') for k in t.kernels]

    assert names() == [FWD, BWD, REDUCE]
    monkeypatch.setenv('SEGFAC_ATTN32_CLASSIC', '1')
    assert names() == [FWD, 'attn_mfma_bwd_fused_kernel<32, 4, true>', REDUCE]
