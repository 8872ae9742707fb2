"""Float64 checks of the norm and column-reduction kernels (csrc/norm.hip, csrc/colreduce.h): LayerNorm forward / backward, BatchNorm
statistics / apply / backward, GRN forward / backward and colsum, each against a plain float64 statement of the operation
(tests/norm_refs.py) at the shapes where the kernels take another path and on inputs that are NOT friendly: a mean of 100 sigma, a
variance far below eps, constant groups, a single outlier, all-zero channels and images.

The bound is the reference's own fp32 error, not a share of the largest element (tests/test_kernels_gpu.py):

    |got - ref64| <= half_ulp_T(ref64) + max(MARGIN * e_ref, FLOOR * 2^-24 * scale)          (norm_refs.compare)

e_ref is measured at run time on the same inputs from the fp32 statement of the operation on the CPU (F.layer_norm, the literal GRN module
and F.gelu with autograd, fp32 `.sum(0)` and the sequential fp32 sum) -- never from the kernel.  MARGIN / FLOOR are 4 / 4 for elementwise
outputs and statistics and 2 / 4 for reductions.  Where a case needs a larger bound the term is DERIVED from the kernel's chain of
additions and written beside the case in norm_refs.py, where `DERIVED` is read (the list is below); CPU tests show for three of them that
the plain fp32 statements need the same terms, with no kernel involved.

BatchNorm: segf_bn_apply and segf_bn_bwd are checked as functions of the mean / rstd that segf_bn_stats wrote; the statistics have their
own check, whose e_ref is the documented algorithm (fp32 sums of x and x^2 combined in float64) -- so the variance is held to what fp32
sums allow, an error that grows as (mean / sigma)^2, and to nothing tighter.

Not covered: the CR_MAX_BLOCKS cap of cr_plan (it needs more than 260 k rows at C = 512, 134 M elements), the fused BatchNorm backward
forms (bn_cls_bwd*), softmax-CE and fp8 quantisation.  cr_plan's channel slabs are covered by C = 768 (three slabs of 32 chunk lanes) and
by C = 2304 / 3080 (two slabs of 256 chunk lanes, the second partly idle).

Observed on an MI355X, the largest (err - half_ulp) / max(e_ref, FLOOR / MARGIN * 2^-24 * scale) per (operation, output); the test fails
above MARGIN:

    operation   output        ratio   allowed   case
    ----------  ------------  ------  --------  ----
    batchnorm   eval.dbeta     0.914         2  bn-offset30-1367x2304-act1 fp32
    batchnorm   eval.dgamma        1         2  bn-tiny-1367x2304-act1 fp32
    batchnorm   eval.dx            1         4  bn-plain-1x72-act1 fp32
    batchnorm   sums.mean       0.92         4  bn-plain-2x72-act1 fp32
    batchnorm   sums.rmean      1.34         4  bn-plain-1367x2304-act1 fp32
    batchnorm   sums.rstd       1.37         4  bn-plain-4101x768-act1 fp32
    batchnorm   sums.rvar       1.57         4  bn-plain-1367x2304-act1 fp32
    batchnorm   mean            1.57         4  bn-plain-150x19-act1 fp32
    batchnorm   rmean           1.52         4  bn-plain-1367x2304-act1 fp32
    batchnorm   rstd            2.72         4  bn-plain-150x19-act1 bf16
    batchnorm   rvar            2.26         4  bn-plain-1367x2304-act1 fp32
    batchnorm   train.dbeta    0.914         2  bn-offset30-1367x2304-act1 fp32
    batchnorm   train.dgamma       1         2  bn-tiny-1367x2304-act1 fp32
    batchnorm   train.dx        1.98         4  bn-offset8-4101x72-act0 fp32
    batchnorm   y               1.97         4  bn-const-4101x768-act1 fp32
    colsum      sum             1.63         2  colsum-positive-300x3080 fp32
    grn         dbeta          0.748         2  grn-plain-1x8-id fp32
    grn         dgamma          1.66         2  grn-plain-1x8-id fp32
    grn         dx              3.01         4  grn-plain-49x40-gelu fp32
    grn         sq              1.69         2  grn-zero_channel-1x8-gelu bf16
    grn         y               2.67         4  grn-big-1367x768-id fp32
    layernorm   dbeta              1         2  ln-plain-5x3072-eps1e-06 fp32
    layernorm   dgamma          1.89         2  ln-plain-5x3072-eps1e-06 fp32
    layernorm   dx              3.03         4  ln-outlier-333x40-eps1e-05 fp32
    layernorm   dxs            0.971         4  ln-fanin-333x40-eps1e-05 fp32
    layernorm   mean            3.92         4  ln-outlier-67x520-eps1e-05 fp32
    layernorm   rstd            3.42         4  ln-outlier-333x40-eps1e-05 bf16
    layernorm   y               3.97         4  ln-plain-16391x512-eps1e-05 fp32

(`sums.*`: segf_bn_stats_from_sums on float64-exact sums rounded to fp32, under the bound of segf_bn_stats.)

The DERIVED terms, each with its derivation in norm_refs.py, and the cases they apply to:
  ln_offset_terms            LayerNorm y, dx, dgamma, class `offset`: the mean is a sum of 100-sigma elements; F.layer_norm's running mean is not
  LN_DX_FLOOR = 8            LayerNorm dx, every case: eight roundings on dx's own way
  ln_dgamma_roundings        LayerNorm dgamma, class `outlier`: one term carries the sum
  bn_apply_affine_term       BatchNorm y, every case: y = act(a x + b) with b = beta - mean a; behind an activation the sizes of pre, not of y
  bn_variance_terms          BatchNorm rstd, running_var, classes `offset8`, `offset30`, `outlier` and rows <= 2: the stated (mean / sigma)^2 contract
  cr_roundings as floor      BatchNorm mean, running_mean, the same three classes; dgamma (+ 3), class `outlier`
  bn_dx_cancellation_term    BatchNorm training dx, class `outlier` and rows <= 2: the three terms of dx cancel
  grn_single_row_term        GRN dx and y at rows_per_sample = 1: one-element groups, differences of larger terms
  grn_gelu_terms             GRN sums and dgamma with pre_gelu: the absolute error of the kernels' erf
With norm_refs.DERIVED = False the issue's bound alone is applied; 74 of the 272 GPU cases are then outside it, none of them by a wrong
computation: the derivations say where each excess comes from, and the step-by-step fp32 statements on the CPU (`*_manual32`) show the
same excesses.
"""
import pytest
import torch
import torch.nn.functional as F

import norm_refs as R

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
gpu = pytest.mark.gpu


def _ids(cases):
    return [c['id'] for c in cases]


def _settle(op, Y, verdicts):
    """Print every figure, then assert."""
    for name, v in verdicts.items():
        print(f'RATIO {op} {name} {Y.case["id"]} {str(Y.dtype).replace("torch.", "")} {v.ratio:.4g}')
    bad = [v.message for v in verdicts.values() if not v.ok]
    assert not bad, '\n'.join(bad)


# ---- CPU: the references against autograd ---------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_layernorm_reference_agrees_with_autograd():
    g = R.X.gen(1)
    x = (torch.randn(37, 40, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma, beta = 1 + 0.5 * torch.randn(40, generator=g), 0.5 * torch.randn(40, generator=g)
    dy, dy2, dres = (torch.randn(37, 40, generator=g, dtype=torch.float64) for _ in range(3))
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(x, (40,), gd, bd, 1e-5)
    y.backward(dy + dy2)
    yr, mean, rstd = R.ln_fwd_ref(x.detach(), gamma, beta, 1e-5)
    b = R.ln_bwd_ref(x.detach(), dy, gamma, 1e-5, dy2, dres)
    assert _rel(yr, y.detach()) <= 1e-12 and _rel(b['dx'], x.grad + dres) <= 1e-12
    assert _rel(b['dgamma'], gd.grad) <= 1e-12 and _rel(b['dbeta'], bd.grad) <= 1e-12
    assert _rel(mean, x.detach().mean(-1)) <= 1e-12 and _rel(rstd, (x.detach().var(-1, unbiased=False) + 1e-5).rsqrt()) <= 1e-12


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('training', [True, False])
def test_batchnorm_reference_agrees_with_autograd(act, training):
    g = R.X.gen(2 + act)
    n, C, rps = 150, 19, 50
    x = (torch.randn(n, C, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma, beta = (1 + 0.5 * torch.randn(C, generator=g)) * 3, 0.5 * torch.randn(C, generator=g)
    cs = torch.rand(3, C, generator=g) + 0.5
    dy = torch.randn(n, C, generator=g, dtype=torch.float64)
    rm0, rv0 = 0.3 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.double().clone(), rv0.double().clone()
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    if not training:                                              # eval mode: the statistics are constants
        mean, rstd = rm.clone(), (rv + 1e-5).rsqrt()
    pre = F.batch_norm(x, rm, rv, gd, bd, training, 0.1, 1e-5)
    y = (pre if act == 0 else F.relu(pre) if act == 1 else F.relu6(pre)) * cs.double()[torch.arange(n) // rps]
    y.backward(dy)
    if training:
        mean, rstd, rmr, rvr = R.bn_stats_ref(x.detach(), 1e-5, rm0, rv0, 0.1)
        assert _rel(rmr, rm) <= 1e-12 and _rel(rvr, rv) <= 1e-12
    yr, _ = R.bn_apply_ref(x.detach(), mean, rstd, gamma, beta, act, cs, rps)
    b = R.bn_bwd_ref(x.detach(), dy, mean, rstd, gamma, beta, act, cs, rps, eval_mode=not training)
    assert _rel(yr, y.detach()) <= 1e-12 and _rel(b['dx'], x.grad) <= 1e-12
    assert _rel(b['dgamma'], gd.grad) <= 1e-12 and _rel(b['dbeta'], bd.grad) <= 1e-12


def test_batchnorm_running_variance_at_one_row():
    x = torch.tensor([[3.0, -2.0]], dtype=torch.float64)
    _, rstd, rm, rv = R.bn_stats_ref(x, 1e-5, torch.zeros(2), torch.ones(2), 0.1)
    assert torch.allclose(rv, torch.full((2,), 0.9, dtype=torch.float64)) and torch.allclose(rstd, torch.full((2,), 1e-5 ** -0.5, dtype=torch.float64))


@pytest.mark.parametrize('pre_gelu', [False, True])
def test_grn_reference_agrees_with_autograd(pre_gelu):
    g = R.X.gen(5)
    B, P, C = 3, 35, 48
    x = torch.randn(B * P, C, generator=g, dtype=torch.float64) * 1.5
    x[:, 5] = 0
    gamma, beta = 0.5 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B * P, C, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = F.gelu(xr) if pre_gelu else xr
    y = R.grn_module(a.reshape(B, 5, 7, C), gd, bd).reshape(-1, C)
    y.backward(dy)
    yr, sq, _ = R.grn_fwd_ref(x, gamma, beta, B, pre_gelu)
    b = R.grn_bwd_ref(x, dy, gamma, B, pre_gelu)
    assert _rel(yr, y.detach()) <= 1e-12 and _rel(b['dx'], xr.grad) <= 1e-12
    assert _rel(b['dgamma'], gd.grad) <= 1e-12 and _rel(b['dbeta'], bd.grad) <= 1e-12
    assert _rel(sq, (a.detach() ** 2).reshape(B, P, C).sum(1)) <= 1e-12
    assert (b['dx'][:, 5] == dy[:, 5] * (R.gelu_grad64(x[:, 5]) if pre_gelu else 1)).all()        # sqrt(0) has gradient 0: K = 0 there


def test_sequential_sum_is_sequential_fp32():
    x = torch.randn(5000, 3, generator=R.X.gen(6)) + 1000
    acc = torch.zeros(3)
    for row in x:
        acc = acc + row
    assert torch.equal(R.seq_sum32(x), acc)
    ref = x.double().sum(0)
    assert ((acc.double() - ref).abs() >= (x.sum(0).double() - ref).abs()).all()


def test_half_ulp_and_comparator():
    ref = torch.tensor([1.0, 1.5, 255.0, 0.0, -3.0], dtype=torch.float64)
    assert R.half_ulp(ref, BF).tolist() == [2.0 ** -8, 2.0 ** -8, 0.5, 0.0, 2.0 ** -7] and not R.half_ulp(ref, F32).any()
    got = R.X.round_bf16(ref * (1 + 2.0 ** -10))
    assert R.compare(got, ref, 0.0, ref.abs(), BF)
    assert not R.compare(got.float() * (1 + 2.0 ** -6), ref, 0.0, ref.abs(), BF)
    assert not R.compare(torch.tensor([float('nan')]), torch.zeros(1, dtype=torch.float64), 1.0, 1.0, F32)
    with pytest.raises(AssertionError, match=r'err / e_ref'):
        R.check(torch.tensor([[1.0, 2.0]]), torch.tensor([[1.0, 2.1]], dtype=torch.float64), 1e-3, 2.0, F32, what='case-name')


# ---- CPU: the input tables ------------------------------------------------------------------------------------------------------------
def test_input_tables_are_well_formed():
    for op, (cases, _, _, _) in R.OPS.items():
        cs = cases()
        assert len({c['id'] for c in cs}) == len(cs)
        for c in cs:
            assert R.case_elements(c) <= R.MAX_ELEMENTS, c['id']
    ln, bn, grn, cs = R.ln_cases(), R.bn_cases(), R.grn_cases(), R.colsum_cases()
    assert max(R.case_elements(c) for c in ln) == 16391 * 512
    for shape in ((333, 40), (67, 520)):
        assert {(c['cls'], c['eps']) for c in ln if (c['rows'], c['C']) == shape and not c['fan']} == {(k, e) for k in R.LN_CLASSES for e in (1e-5, 1e-6)}
    assert {(c['rows'], c['C']) for c in ln if c['cls'] == 'plain'} >= {s[:2] for s in R.LN_PLAIN_SHAPES} and any(c['fan'] for c in ln)
    assert {(c['rows'], c['C'], c['cls']) for c in bn if c['act'] == 1} >= {(r, C, k) for r, C in R.BN_SHAPES for k in R.BN_CLASSES}
    assert {(c['cls'], c['act']) for c in bn if (c['rows'], c['C']) == (4101, 72)} == {(k, a) for k in R.BN_CLASSES for a in (0, 1, 2)}
    assert all(c['rps'] * 3 == c['rows'] for c in bn if c['rows'] % 3 == 0) and any(c['rps'] == 1367 for c in bn)
    assert {(c['rps'], c['C'], c['cls'], c['pre_gelu']) for c in grn} == {(r, C, k, p) for r, C in R.GRN_SHAPES for k in R.GRN_CLASSES for p in (False, True)}
    assert {(c['rows'], c['cols'], c['cls']) for c in cs} == {(r, C, k) for r, C in R.COLSUM_SHAPES for k in R.COLSUM_CLASSES}
    # what the classes promise
    x = R.ln_inputs(next(c for c in ln if c['cls'] == 'const'), BF)['x']
    assert (x == x[:, :1]).all() and x[:, 0].unique().numel() > 10
    x = R.ln_inputs(next(c for c in ln if c['cls'] == 'tiny'), F32)['x']
    assert x.var(-1, unbiased=False).max() < 1e-5
    x = R.bn_inputs(next(c for c in bn if c['cls'] == 'outlier'), F32)
    assert ((x['x'] == 50).sum(0) == 1).all() and x['gamma'][x['gamma'].numel() // 2] == 0
    x = R.grn_inputs(next(c for c in grn if c['cls'] == 'zero_image' and c['rps'] == 49), F32)['x']
    assert not x[49:98].any() and x[:49].any()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_kink_cap(dtype):
    """At most 0.1 % of a tensor lies in the zone around a ReLU / ReLU6 kink that the dx comparison leaves out."""
    for case in R.bn_cases():
        if case['act'] == 0:
            continue
        Y = R.bn_yard(case, dtype)
        mean, rstd = Y.given if Y.given is not None else Y.statement_stats
        _, pre = R.bn_apply_ref(Y.inp['x'], mean, rstd, Y.inp['gamma'], Y.inp['beta'], 0)
        share = R.kink_zone(pre, case['act']).double().mean().item()
        assert share <= R.KINK_CAP, (case['id'], share)
    Y = R.bn_yard(next(c for c in R.bn_cases() if c['cls'] == 'lattice' and c['act'] == 2), dtype)
    pre = Y.inp['x'] * Y.inp['gamma'].double() + Y.inp['beta'].double()
    assert (pre == 6).sum() > 20 and (pre == 0).sum() > 20 and not R.kink_zone(pre, 2).any()


# ---- CPU: every mutant fails, the unmutated statements pass ---------------------------------------------------------------------------
def _statement(op, Y, mut=None):
    _, _, manual, _ = R.OPS[op]
    return manual(Y.inp, Y.case, Y.dtype, mut, **({'given': Y.given} if op == 'bn' else {}))


@pytest.mark.parametrize('op', list(R.OPS))
def test_unmutated_statement_is_accepted_on_every_input(op):
    cases, yard, _, judge = R.OPS[op]
    for case in cases():
        for dtype in DTYPES:
            Y = yard(case, dtype)
            bad = [v.message for v in judge(Y, _statement(op, Y)).values() if not v.ok]
            assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', list(R.MUTANTS))
def test_every_mutant_fails(name):
    """Each wrong computation, in fp32 on the CPU on the GPU tests' own inputs, is rejected on at least one of them -- by outputs on which
    the unmutated statement of the same inputs is accepted."""
    rejected = []
    for op, tag, selectors, outputs in R.MUTANTS[name]:
        cases, yard, _, judge = R.OPS[op]
        chosen = [c for c in cases() if any(s in c['id'] for s in selectors)]
        assert chosen, (name, selectors)
        for case in chosen:
            for dtype in ([BF] if tag in R.BF16_ONLY_MUTANTS else DTYPES):
                Y = yard(case, dtype)
                clean = judge(Y, _statement(op, Y), only=outputs)
                assert clean and all(clean.values()), (name, case['id'], [v.message for v in clean.values() if not v.ok])
                if not all(judge(Y, _statement(op, Y, tag), only=outputs).values()):
                    rejected.append((op, case['id'], dtype))
        assert any(r[0] == op for r in rejected), f'{name}: the {op} mutant {tag} passes on {[c["id"] for c in chosen]}'
    assert rejected


def test_plain_two_pass_fp32_needs_the_offset_term(monkeypatch):
    """The reason for norm_refs.ln_offset_terms, without any kernel: at mean / sigma = 100 the plain two-pass fp32 statement (sum, scale,
    centre) is outside the undivided bound, whose e_ref comes from F.layer_norm's running mean."""
    case = next(c for c in R.ln_cases() if c['id'].startswith('ln-offset-333x40-eps1e-05'))
    monkeypatch.setattr(R, 'DERIVED', False)
    Y = R.ln_yard(case, F32)
    v = R.ln_judge(Y, R.ln_manual32(Y.inp, case, F32), only=('y',))['y']
    assert not v.ok and v.ratio > 4
    monkeypatch.setattr(R, 'DERIVED', True)
    Y = R.ln_yard(case, F32)
    assert R.ln_judge(Y, R.ln_manual32(Y.inp, case, F32), only=('y',))['y'].ok


def test_plain_fp32_layernorm_dx_floor(monkeypatch):
    """The reason for norm_refs.LN_DX_FLOOR, without any kernel: the plain two-pass fp32 statement is outside the floor of 4 on one
    element of the tables."""
    case = next(c for c in R.ln_cases() if c['id'] == 'ln-outlier-333x40-eps1e-06')
    monkeypatch.setattr(R, 'DERIVED', False)
    Y = R.ln_yard(case, F32)
    v = R.ln_judge(Y, R.ln_manual32(Y.inp, case, F32), only=('dx',))['dx']
    assert not v.ok and 4 < v.ratio < 5


def test_plain_fp32_grn_needs_the_single_row_term(monkeypatch):
    """The reason for norm_refs.grn_single_row_term, without any kernel: one-element groups, a difference of two larger terms."""
    case = next(c for c in R.grn_cases() if c['id'] == 'grn-tiny-1x8-id')
    monkeypatch.setattr(R, 'DERIVED', False)
    Y = R.grn_yard(case, F32)
    assert not R.grn_judge(Y, R.grn_manual32(Y.inp, case, F32), only=('dx',))['dx'].ok
    monkeypatch.setattr(R, 'DERIVED', True)
    Y = R.grn_yard(case, F32)
    assert R.grn_judge(Y, R.grn_manual32(Y.inp, case, F32), only=('dx',))['dx'].ok


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    from segmentation_factory_amd import hip
    hip.lib()
    return hip


def _dev(t, dtype=F32):
    """A CPU tensor (float64 activations are already rounded to `dtype`: the cast is exact) on the device."""
    return None if t is None else t.to(dtype).cuda().contiguous()


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _ran(trace, *names):
    assert trace.launches > 0, 'no kernel was launched'
    for n in names:
        assert any(n in k for k in trace.kernels), (n, trace.kernels)


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', R.ln_cases(), ids=_ids(R.ln_cases()))
def test_layernorm(hip, case, dtype):
    Y = R.ln_yard(case, dtype)
    i = Y.inp
    x, dy, gamma, beta = _dev(i['x'], dtype), _dev(i['dy'], dtype), _dev(i['gamma']), _dev(i['beta'])
    with hip.trace() as t:
        y, mean, rstd = hip.layernorm_fwd(x, gamma, beta, case['eps'])
        dx, dg, db = hip.layernorm_bwd(x, dy, gamma, mean, rstd, dy2=_dev(i['dy2'], dtype), dres=_dev(i['dres'], dtype),
                                       rscale=_dev(i['rscale']), rows_per_group=R.LN_RPG)
    torch.cuda.synchronize()
    _ran(t, 'ln_fwd_kernel', 'ln_bwd_kernel', 'colreduce_finalize')
    assert (dx.scaled is not None) == case['fan']
    got = dict(y=_cpu(y), mean=_cpu(mean), rstd=_cpu(rstd), dx=_cpu(dx), dgamma=_cpu(dg), dbeta=_cpu(db), dxs=_cpu(dx.scaled))
    _settle('layernorm', Y, R.ln_judge(Y, got))


def _accepts_or_refuses(hip, fn, C):
    """An entry point may refuse a channel count that is no multiple of 8, with SEGF_ERR_SHAPE; any other failure is one."""
    try:
        return fn()
    except RuntimeError as e:
        assert C % 8 != 0 and f'code {hip.ERR_SHAPE} ' in str(e), e
        return None


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', R.bn_cases(), ids=_ids(R.bn_cases()))
def test_batchnorm(hip, case, dtype):
    Y = R.bn_yard(case, dtype)
    i, C, rows, act, rps = Y.inp, case['C'], case['rows'], case['act'], max(case['rps'], 1)
    x, dy, gamma, beta, cs = _dev(i['x'], dtype), _dev(i['dy'], dtype), _dev(i['gamma']), _dev(i['beta']), _dev(i['chan_scale'])
    rm, rv, rm2, rv2 = _dev(i['rmean0']), _dev(i['rvar0']), _dev(i['rmean0']), _dev(i['rvar0'])
    exact_sums = _dev(torch.stack([i['x'].sum(0), (i['x'] * i['x']).sum(0)]))            # float64 sums, rounded once to fp32
    got, from_sums = {}, {}
    with hip.trace() as t:
        if Y.given is None:
            st = _accepts_or_refuses(hip, lambda: hip.bn_stats(x, rm, rv, R.BN_MOMENTUM, R.BN_EPS), C)
            st2 = _accepts_or_refuses(hip, lambda: hip.bn_stats_from_sums(exact_sums, rows, rm2, rv2, R.BN_MOMENTUM, R.BN_EPS), C)
            assert st is not None, 'segf_bn_stats is the source of the statistics of the later steps'
            got.update(mean=_cpu(st[0]), rstd=_cpu(st[1]), rmean=_cpu(rm), rvar=_cpu(rv))
            if st2 is not None:
                from_sums.update(mean=_cpu(st2[0]), rstd=_cpu(st2[1]), rmean=_cpu(rm2), rvar=_cpu(rv2))
            mean, rstd = st
        else:
            mean, rstd = _dev(Y.given[0]), _dev(Y.given[1])
        y = _accepts_or_refuses(hip, lambda: hip.bn_apply(x, mean, rstd, gamma, beta, act, cs, rps), C)
        got['y'] = _cpu(y)
        for name, mode in (('train', False), ('eval', True)):
            r = _accepts_or_refuses(hip, lambda: hip.bn_bwd(x, dy, mean, rstd, gamma, beta, act, cs, rps, mode), C)
            got[name] = None if r is None else dict(dx=_cpu(r[0]), dgamma=_cpu(r[1]), dbeta=_cpu(r[2]))
    torch.cuda.synchronize()
    _ran(t, *(('bn_finalize_kernel', 'BnStatF') if Y.given is None else ()), 'bn_apply_kernel', 'BnBwdF', 'bn_bwd_apply_kernel')
    verdicts = R.bn_judge(Y, got)
    verdicts.update({f'from_sums.{k}': v for k, v in R.judge(Y.entries, from_sums, f'{case["id"]} {dtype} from exact sums').items()})
    _settle('batchnorm', Y, verdicts)


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', R.grn_cases(), ids=_ids(R.grn_cases()))
def test_grn(hip, case, dtype):
    Y = R.grn_yard(case, dtype)
    i = Y.inp
    x, dy, gamma, beta = _dev(i['x'], dtype), _dev(i['dy'], dtype), _dev(i['gamma']), _dev(i['beta'])
    with hip.trace() as t:
        y, sq = hip.grn_fwd(x, gamma, beta, R.GRN_B, case['rps'], pre_gelu=case['pre_gelu'])
        dx, dg, db = hip.grn_bwd(x, dy, gamma, sq, R.GRN_B, case['rps'], pre_gelu=case['pre_gelu'])
    torch.cuda.synchronize()
    _ran(t, 'GrnSqF', 'GrnBwdF', 'grn_coef_kernel', 'grn_apply_kernel', 'grn_param_grads_kernel')
    _settle('grn', Y, R.grn_judge(Y, dict(y=_cpu(y), sq=_cpu(sq), dx=_cpu(dx), dgamma=_cpu(dg), dbeta=_cpu(db))))


@gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', R.colsum_cases(), ids=_ids(R.colsum_cases()))
def test_colsum(hip, case, dtype):
    Y = R.colsum_yard(case, dtype)
    with hip.trace() as t:
        s = hip.colsum(_dev(Y.inp['x'], dtype))
    torch.cuda.synchronize()
    _ran(t, 'ColsumF', 'colreduce_finalize')
    _settle('colsum', Y, R.colsum_judge(Y, dict(sum=_cpu(s))))
